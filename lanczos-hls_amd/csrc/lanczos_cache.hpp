// lanczos_cache.hpp -- host-side lifetime of what a context keeps on the device: retire lists, the workgroup-table cache of
// k_march, and the recency order of the plan cache.  No kernels here.
//
// Rule: a device block (or the page-locked source of an asynchronous upload) that launches still in flight may be reading is
// never freed on the spot and never with a device-wide sync: an event is recorded on every stream the block was used on, and
// the block is freed by a later call once those events have completed -- or at destruction, after the owner has drained the
// device.  If an event cannot be recorded (a stream the caller has destroyed in the meantime) the block is NOT treated as
// drained: it stays until the owner's final reap(true) behind a device-wide sync (lanczos_destroy).
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
#include <vector>

#ifndef LZ_CACHE_TEST_STUBS
#include <hip/hip_runtime.h>
#endif

namespace lz {

struct Retired {
    std::vector<void*> dev, host;   // hipFree / hipHostFree
    std::vector<hipEvent_t> ev;
    bool unrecorded = false;        // an event could not be recorded: only a reap behind a device-wide sync may free this
};
struct RetireList {
    std::vector<Retired> list;
    void retire(const std::vector<void*>& dev, const std::vector<void*>& host, const std::vector<hipStream_t>& streams) {
        Retired r;
        r.dev = dev;
        r.host = host;
        for (hipStream_t st : streams) {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess && hipEventRecord(e, st) == hipSuccess) {
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
// true while `s` is being captured into a graph (and when that cannot be told): work queued on it now does not run now
inline bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
}
inline void note_stream(std::vector<hipStream_t>& v, hipStream_t s) {
    if (std::find(v.begin(), v.end(), s) == v.end()) v.push_back(s);
}

// recency order of a bounded cache: touch() on every hit and insert, oldest() names the entry to evict
template <typename Key>
struct LruOrder {
    std::vector<Key> order;   // least recently used first
    void touch(const Key& k) {
        for (size_t i = 0; i < order.size(); i++)
            if (memcmp(&order[i], &k, sizeof(Key)) == 0) {
                order.erase(order.begin() + i);
                break;
            }
        order.push_back(k);
    }
    bool empty() const { return order.empty(); }
    Key pop_oldest() {
        Key k = order.front();
        order.erase(order.begin());
        return k;
    }
};

// device copies of the workgroup tables a context has used (callers serialise per context).  A table is built once per launch
// shape into page-locked memory and uploaded asynchronously on the stream of its first launch; launches on other streams wait
// for that upload by event.  Bounded: the least recently used shape is retired when the 65th arrives.
//
// Stream capture: a copy queued on a stream that is being captured becomes a graph node and moves nothing until the graph is
// replayed -- perhaps never -- so a table first needed by a captured launch goes up eagerly instead: a copy on the cache's
// private stream and a wait for it.  The item is valid from the moment it is cached and carries no `uploaded` event (nothing is
// ever recorded on, queried from or waited for on a capturing stream).  A table a captured launch has used may be named by a
// live graph: eviction moves its blocks to `kept`, which only release_all() frees -- a graph must not outlive its context.
template <typename Entry>
struct WgTabCacheT {
    static constexpr size_t kMaxItems = 64;
    struct Item {
        long long key[8];
        Entry* dev = nullptr;
        Entry* host = nullptr;             // page-locked source of the upload (stays valid while the copy is in flight)
        int n = 0, segs = 1;
        bool balanced = false;
        bool mode_a = false;               // march_build_table's branch: one workgroup per CU slot (A) or whole chunks (B)
        hipEvent_t uploaded = nullptr;     // recorded behind the upload; none where the upload was eager (complete)
        hipStream_t upload_stream = nullptr;
        std::vector<hipStream_t> streams;  // streams this shape was uploaded / launched on (not captured ones)
        bool captured = false;             // a captured launch has used it
    };
    std::vector<Item> items;               // least recently used first
    RetireList retired;
    std::vector<void*> kept_dev, kept_host;   // blocks of evicted items a live graph may still name
    hipStream_t eager = nullptr;              // private stream of the eager uploads, created on first need
    hipError_t eager_stream(hipStream_t* s) {
        hipError_t e = hipSuccess;
        if (!eager) e = hipStreamCreateWithFlags(&eager, hipStreamNonBlocking);
        *s = eager;
        return e;
    }
    // every use of an item by a launch on `stream` goes through here: orders the launch behind the upload and remembers what
    // has to drain before the item's blocks may go
    hipError_t use(Item* it, hipStream_t stream) {
        if (stream_capturing(stream)) {
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
    // lanczos_last_march_table: the shape of the last k_march launch (march_issue_t notes it where it launches, the entry points
    // clear it when a call begins).  A key, not a pointer: items move on every insert.
    long long last_key[8] = {};
    bool last_valid = false;
    void note_last(const long long (&key)[8]) {
        memcpy(last_key, key, sizeof(key));
        last_valid = true;
    }
    const Item* last() const {   // (no recency update: a report is not a use)
        if (!last_valid) return nullptr;
        for (const Item& it : items)
            if (memcmp(it.key, last_key, sizeof(last_key)) == 0) return &it;
        return nullptr;
    }

    Item* find(const long long (&key)[8]) {
        for (size_t i = 0; i < items.size(); i++)
            if (memcmp(items[i].key, key, sizeof(key)) == 0) {
                if (i + 1 != items.size()) std::rotate(items.begin() + i, items.begin() + i + 1, items.end());  // most recent last
                return &items.back();
            }
        return nullptr;
    }
    // uploads `tab` on `stream` (eagerly on the private stream if `stream` is being captured) and returns the new item
    // (nullptr + *err on failure).  Pointers to items are valid until the next insert().
    Item* insert(const long long (&key)[8], const std::vector<Entry>& tab, int n, int segs, bool balanced, hipStream_t stream,
                 hipError_t* err, bool mode_a = false) {
        retired.reap(false);
        Item it;
        memcpy(it.key, key, sizeof(key));
        it.n = n, it.segs = segs, it.balanced = balanced, it.mode_a = mode_a;
        const size_t bytes = sizeof(Entry) * tab.size();
        const bool capturing = stream_capturing(stream);   // hipStreamIsCapturing: the upload below must not become a graph node
        hipStream_t up = stream;
        hipError_t e = capturing ? eager_stream(&up) : hipSuccess;
        if (e != hipSuccess) {
            *err = e;
            return nullptr;
        }
        e = hipMalloc((void**)&it.dev, bytes);
        if (e == hipSuccess) e = hipHostMalloc((void**)&it.host, bytes, hipHostMallocDefault);
        if (e == hipSuccess && !capturing) e = hipEventCreateWithFlags(&it.uploaded, hipEventDisableTiming);
        if (e == hipSuccess) {
            memcpy(it.host, tab.data(), bytes);
            e = hipMemcpyAsync(it.dev, it.host, bytes, hipMemcpyHostToDevice, up);  // stream-ordered in front of the first launch
        }
        if (e == hipSuccess) e = capturing ? hipStreamSynchronize(up) : hipEventRecord(it.uploaded, stream);
        if (e != hipSuccess) {
            // the copy may have been queued: nothing it touches is freed before that stream has drained
            if (it.uploaded) (void)hipEventDestroy(it.uploaded);
            retired.retire({it.dev}, {it.host}, {up});
            *err = e;
            return nullptr;
        }
        if (capturing) {
            it.captured = true;             // complete: no event, no upload stream to stay behind
        } else {
            it.upload_stream = stream;
            it.streams.push_back(stream);   // the upload itself reads `host` and writes `dev` on this stream
        }
        if (items.size() >= kMaxItems) drop(0);  // bounded: the least recently used shape goes (freed once its launches have drained)
        items.push_back(it);
        *err = hipSuccess;
        return &items.back();
    }
    void drop(size_t i) {
        Item& it = items[i];
        if (it.captured) {
            kept_dev.push_back(it.dev);
            kept_host.push_back(it.host);
        } else {
            retired.retire({it.dev}, {it.host}, it.streams);
        }
        if (it.uploaded) (void)hipEventDestroy(it.uploaded);
        items.erase(items.begin() + i);
    }
    // the owner has made sure that nothing is in flight any more (lanczos_destroy: after the device has drained, before the
    // context's streams go): free everything now -- no events on streams that may be gone by the time a destructor runs
    void release_all() {
        retired.reap(true);
        for (Item& it : items) {
            (void)hipFree(it.dev);
            (void)hipHostFree(it.host);
            if (it.uploaded) (void)hipEventDestroy(it.uploaded);
        }
        items.clear();
        for (void* p : kept_dev) (void)hipFree(p);
        for (void* p : kept_host) (void)hipHostFree(p);
        kept_dev.clear();
        kept_host.clear();
        if (eager) (void)hipStreamDestroy(eager);
        eager = nullptr;
    }
    ~WgTabCacheT() { release_all(); }
};

}  // namespace lz
