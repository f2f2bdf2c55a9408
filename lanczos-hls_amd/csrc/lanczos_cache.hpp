// lanczos_cache.hpp -- the one lifetime policy of every device block a context caches: the retire list, the bounded upload
// cache (tap-table plans, k_march's workgroup tables, the resize axes are instances of it) and the growable scratch block.
// No kernels here.
//
// Rule: a device block (or the page-locked source of an asynchronous upload) that launches still in flight may be reading is
// never freed on the spot and never with a device-wide sync: an event is recorded on every stream the block was used on, and
// the block is freed by a later call once those events have completed -- or at destruction, after the owner has drained the
// device.  If an event cannot be recorded (a stream the caller has destroyed in the meantime, or one that is being captured by
// now: the record would become a graph node) the block is NOT treated as drained: it stays until the owner's final reap(true)
// behind a device-wide sync (lanczos_destroy).  A block a captured launch has used may be named by a live graph: it is never
// retired but `kept` until the context goes -- a graph must not outlive its context.
//
// Why the page-locked source exists at all (DESIGN.md 9, round-3 harness crash): an intermediate state of round 3 uploaded the
// table with hipMemcpyAsync straight out of the std::vector that march_build_table had filled -- pageable memory whose copy the
// runtime may finish after the call has returned -- and the vector died at the end of the scope.  The copy then reads freed
// memory: mostly still mapped (silent), sometimes not (SIGSEGV with nothing on stdout, seen once in gpurun_out/r3g).  The
// committed code copies the table into a page-locked block owned by the cache item and frees it only through the retire list.
//
// The host logic is exercised without a GPU by tests/native/cache_lifetime_check.cpp (-fsanitize=address,undefined), which
// compiles this header against counting stand-ins for the few HIP calls it makes (LZ_CACHE_TEST_STUBS).
#pragma once
#include <algorithm>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#ifndef LZ_CACHE_TEST_STUBS
#include <hip/hip_runtime.h>
#endif

namespace lz {

// true while `s` is being captured into a graph (and when that cannot be told): work queued on it now does not run now
inline bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
}
inline void note_stream(std::vector<hipStream_t>& v, hipStream_t s) {
    if (std::find(v.begin(), v.end(), s) == v.end()) v.push_back(s);
}

struct Retired {
    std::vector<void*> dev, host;   // hipFree / hipHostFree
    std::vector<hipEvent_t> ev;
    bool unrecorded = false;        // an event could not be recorded: only a reap behind a device-wide sync may free this
};
struct RetireList {
    std::vector<Retired> list;
    // `streams` were noted when they were used, perhaps long ago: one of them may be capturing by now and gets no event
    void retire(const std::vector<void*>& dev, const std::vector<void*>& host, const std::vector<hipStream_t>& streams) {
        Retired r;
        r.dev = dev;
        r.host = host;
        for (hipStream_t st : streams) {
            hipEvent_t e = nullptr;
            if (!stream_capturing(st) && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess &&
                hipEventRecord(e, st) == hipSuccess) {
                r.ev.push_back(e);
            } else {
                if (e) (void)hipEventDestroy(e);
                r.unrecorded = true;
            }
        }
        list.push_back(r);
    }
    // wait == false: free what has provably drained.  wait == true: the caller has drained the device (or accepts waiting on
    // every recorded event); everything goes.
    void reap(bool wait) {
        for (size_t i = 0; i < list.size();) {
            bool done = !list[i].unrecorded || wait;
            for (hipEvent_t e : list[i].ev) {
                if (wait) (void)hipEventSynchronize(e);
                else if (hipEventQuery(e) != hipSuccess) done = false;
            }
            if (!done) {
                i++;
                continue;
            }
            for (hipEvent_t e : list[i].ev) (void)hipEventDestroy(e);
            for (void* p : list[i].dev) (void)hipFree(p);
            for (void* p : list[i].host) (void)hipHostFree(p);
            list.erase(list.begin() + i);
        }
    }
    ~RetireList() { reap(true); }
};

// What the caches and scratch blocks of one context share (the context owns it and hands it to them; callers serialise per
// context): where their blocks go when they are replaced, and the private stream of the eager uploads.
struct Lifetime {
    RetireList retired;                       // replaced blocks that launches in flight may still read
    std::vector<void*> kept_dev, kept_host;   // replaced blocks a live graph may still name: only release_all() frees them
    hipStream_t eager = nullptr;              // created on first need
    hipError_t eager_stream(hipStream_t* s) {
        hipError_t e = hipSuccess;
        if (!eager) e = hipStreamCreateWithFlags(&eager, hipStreamNonBlocking);
        *s = eager;
        return e;
    }
    // a replaced block: kept if a captured launch has used it, retired behind `streams` otherwise
    void replace(void* dev, void* host, bool captured, const std::vector<hipStream_t>& streams) {
        if (!captured) return retired.retire({dev}, {host}, streams);
        if (dev) kept_dev.push_back(dev);
        if (host) kept_host.push_back(host);
    }
    // the owner has made sure that nothing is in flight any more (lanczos_destroy: after the device has drained, before the
    // context's streams go): free everything now -- no events on streams that may be gone by the time a destructor runs
    void release_all() {
        retired.reap(true);
        for (void* p : kept_dev) (void)hipFree(p);
        for (void* p : kept_host) (void)hipHostFree(p);
        kept_dev.clear();
        kept_host.clear();
        if (eager) (void)hipStreamDestroy(eager);
        eager = nullptr;
    }
    ~Lifetime() { release_all(); }
};

// how an item's block reaches the device
enum class Upload {
    // asynchronously on the stream of the first call that needs it, out of a page-locked source the item owns; an `uploaded`
    // event orders other streams behind it.  A stream that is being captured would turn the copy and the event into graph nodes
    // that run only when the graph is replayed, perhaps never, while the item is cached as valid: there the upload is eager
    // instead (and the item still owns its page-locked source)
    on_stream,
    // always a copy on the private stream and a wait for it, straight out of the caller's source: complete when insert()
    // returns, no event, no page-locked block
    eager,
};

// A bounded cache of device blocks that are built on the host and uploaded once.  Key: trivially copyable, zero-initialised by
// the caller, compared by memcmp.  Items are allocated one by one: a pointer stays valid until that item is evicted, and an
// insert evicts the least recently used item, never the one touched just before it (max_items >= 2).
template <typename Key, typename Payload>
struct UploadCache {
    struct Item : Payload {
        Key key;
        void* dev_block = nullptr;
        void* host_block = nullptr;        // page-locked source of the upload (stays valid while the copy is in flight)
        hipEvent_t uploaded = nullptr;     // recorded behind the upload; none where the upload was eager (complete)
        hipStream_t upload_stream = nullptr;
        std::vector<hipStream_t> streams;  // streams the block was uploaded / used on (not captured ones)
        bool captured = false;             // a captured launch has used it
        explicit Item(Payload&& v) : Payload(std::move(v)) {}
    };
    Lifetime* const life;
    const size_t max_items;
    std::vector<Item*> items;              // least recently used first
    UploadCache(Lifetime* l, size_t bound) : life(l), max_items(bound) {}
    UploadCache(const UploadCache&) = delete;

    const Item* peek(const Key& key) const {   // no recency update (a report is not a use)
        for (const Item* it : items)
            if (memcmp(&it->key, &key, sizeof(Key)) == 0) return it;
        return nullptr;
    }
    Item* find(const Key& key) {
        for (size_t i = 0; i < items.size(); i++)
            if (memcmp(&items[i]->key, &key, sizeof(Key)) == 0) {
                std::rotate(items.begin() + i, items.begin() + i + 1, items.end());   // most recent last
                return items.back();
            }
        return nullptr;
    }
    // every use of an item by a launch on `stream` goes through here: orders the launch behind the upload and remembers what
    // has to drain before the item's block may go.  Nothing is recorded on, queried from or waited for on a capturing stream.
    hipError_t use(Item* it, hipStream_t stream, bool capturing) {
        if (capturing) {
            // (an upload still in flight on another stream is waited for here: the graph gets no node for it)
            if (it->uploaded && hipEventQuery(it->uploaded) != hipSuccess) {
                const hipError_t e = hipEventSynchronize(it->uploaded);
                if (e != hipSuccess) return e;
            }
            it->captured = true;
            return hipSuccess;
        }
        if (it->uploaded && stream != it->upload_stream && hipEventQuery(it->uploaded) != hipSuccess) {
            const hipError_t e = hipStreamWaitEvent(stream, it->uploaded, 0);  // another stream: behind the upload
            if (e != hipSuccess) return e;
        }
        note_stream(it->streams, stream);
        return hipSuccess;
    }
    hipError_t use(Item* it, hipStream_t stream) { return use(it, stream, stream_capturing(stream)); }
    // uploads `bytes` of `src` and returns the new item, most recent (nullptr + *err on failure)
    Item* insert(const Key& key, Payload&& v, const void* src, size_t bytes, hipStream_t stream, Upload mode, hipError_t* err) {
        life->retired.reap(false);
        Item* it = new (std::nothrow) Item(std::move(v));
        if (!it) {
            *err = hipErrorOutOfMemory;
            return nullptr;
        }
        it->key = key;
        const bool capturing = stream_capturing(stream);   // hipStreamIsCapturing: the upload below must not become a graph node
        const bool eager = capturing || mode == Upload::eager, pinned = mode == Upload::on_stream;
        hipStream_t up = stream;
        hipError_t e = eager ? life->eager_stream(&up) : hipSuccess;
        if (e == hipSuccess) e = hipMalloc(&it->dev_block, bytes);
        if (e == hipSuccess && pinned) e = hipHostMalloc(&it->host_block, bytes, hipHostMallocDefault);
        if (e == hipSuccess && !eager) e = hipEventCreateWithFlags(&it->uploaded, hipEventDisableTiming);
        if (e == hipSuccess) {
            if (pinned) memcpy(it->host_block, src, bytes);
            // (not eager: stream-ordered in front of the first launch)
            e = hipMemcpyAsync(it->dev_block, pinned ? it->host_block : src, bytes, hipMemcpyHostToDevice, up);
        }
        if (e == hipSuccess) e = eager ? hipStreamSynchronize(up) : hipEventRecord(it->uploaded, stream);
        if (e != hipSuccess) {
            // the copy may have been queued: nothing it touches is freed before that stream has drained
            if (it->uploaded) (void)hipEventDestroy(it->uploaded);
            life->retired.retire({it->dev_block}, {it->host_block}, {up});
            delete it;
            *err = e;
            return nullptr;
        }
        if (capturing) it->captured = true;
        if (!eager) {
            it->upload_stream = stream;
            it->streams.push_back(stream);   // the upload itself reads `host_block` and writes `dev_block` on this stream
        }
        if (items.size() >= max_items) evict(0);   // bounded (the block is freed once its launches have drained)
        items.push_back(it);
        *err = hipSuccess;
        return it;
    }
    void evict(size_t i) {
        Item* it = items[i];
        life->replace(it->dev_block, it->host_block, it->captured, it->streams);
        if (it->uploaded) (void)hipEventDestroy(it->uploaded);
        delete it;
        items.erase(items.begin() + i);
    }
    // the owner has drained the device (Lifetime::release_all follows)
    void release_all() {
        for (Item* it : items) {
            (void)hipFree(it->dev_block);
            (void)hipHostFree(it->host_block);
            if (it->uploaded) (void)hipEventDestroy(it->uploaded);
            delete it;
        }
        items.clear();
    }
    ~UploadCache() { release_all(); }
};

// A block of context scratch that grows on demand and never shrinks.  Every stream that touches it is noted on it; the block a
// larger one replaces goes the way of every replaced block (Lifetime::replace).
struct ScratchBlock {
    void* p = nullptr;
    size_t bytes = 0;
    bool captured = false;               // used by a captured launch: a live graph may still hold it
    std::vector<hipStream_t> streams;
    ScratchBlock() = default;
    ScratchBlock(const ScratchBlock&) = delete;
    void note(hipStream_t stream, bool capturing) {
        if (capturing) captured = true;
        else note_stream(streams, stream);
    }
    // at least `need` bytes, about to be used on `stream`.  A failed allocation leaves the block empty and usable
    hipError_t reserve(Lifetime* life, size_t need, hipStream_t stream, bool capturing) {
        if (bytes < need) {
            if (p) life->replace(p, nullptr, captured, streams);
            p = nullptr;
            bytes = 0;
            captured = false;
            streams.clear();
            const hipError_t e = hipMalloc(&p, need);
            if (e != hipSuccess) {
                p = nullptr;
                return e;
            }
            bytes = need;
        }
        note(stream, capturing);
        return hipSuccess;
    }
    ~ScratchBlock() { (void)hipFree(p); }   // the owner has drained the device
};

}  // namespace lz
