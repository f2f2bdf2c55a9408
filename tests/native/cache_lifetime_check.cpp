// tests/native/cache_lifetime_check.cpp -- the host-side lifetime logic of lanczos_cache.hpp without a GPU, under
// -fsanitize=address,undefined: the retire list, the bounded upload cache in both upload modes (the plans, the workgroup tables
// and the resize axes are instances of it) and the growable scratch block.
//
// The handful of HIP calls the header makes are replaced by a small model of streams: work queued on a stream (an asynchronous
// copy, an event record) completes only when the test drains that stream, and the model objects to
//   * freeing a block that a queued copy still reads or writes (the round-3 harness crash: DESIGN.md 9),
//   * freeing a block twice, leaking one, recording on a destroyed stream (reported as an error code, as HIP does),
//   * queueing a copy, an event record or a wait on a stream that is being captured into a graph,
//   * a copy that reads a caller's own (pageable) source after the call that took it has returned.
// Round 3's verdict asked for exactly this: create -> many shapes -> destroy of the cache + RetireList with stubbed events.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

// ------------------------------------------------------------------------------------------------ the model
typedef int hipError_t;
static const hipError_t hipSuccess = 0, hipErrorNotReady = 600, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2;
struct StubStream {
    bool alive = true;
    bool capturing = false;                                // work queued now would become graph nodes: nothing may be queued
    std::vector<int> pending_events;                       // ids of events recorded and not yet reached
    std::vector<std::pair<const void*, const void*>> copies;  // (dst, src) of copies queued and not yet done
};
struct StubEvent {
    int id;
    bool recorded = false, done = false;
};
typedef StubStream* hipStream_t;
typedef StubEvent* hipEvent_t;
static const unsigned hipEventDisableTiming = 2, hipHostMallocDefault = 0, hipStreamNonBlocking = 1;
enum hipStreamCaptureStatus { hipStreamCaptureStatusNone = 0, hipStreamCaptureStatusActive = 1 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };

static std::set<void*> g_dev, g_host;
static std::set<const void*> g_pageable;   // a caller's own source of an eager upload, for as long as the caller keeps it alive
static std::map<int, StubEvent*> g_events;
static std::vector<StubStream*> g_streams;
static int g_next_event = 1, g_fail_host_malloc_at = -1, g_host_mallocs = 0, g_fail_copy_at = -1, g_copies = 0, g_violations = 0;
static int g_fail_dev_malloc_at = -1, g_dev_mallocs = 0, g_fail_record_at = -1, g_records = 0;

static void violation(const char* what) {
    printf("VIOLATION: %s\n", what);
    g_violations++;
}
static bool in_flight(const void* p) {
    for (StubStream* s : g_streams)
        for (auto& c : s->copies)
            if (c.first == p || c.second == p) return true;
    return false;
}
static hipError_t hipMalloc(void** p, size_t n) {
    if (g_dev_mallocs++ == g_fail_dev_malloc_at) return hipErrorOutOfMemory;   // (*p left as it was, as HIP leaves it)
    *p = malloc(n ? n : 1);
    g_dev.insert(*p);
    return hipSuccess;
}
static hipError_t hipHostMalloc(void** p, size_t n, unsigned) {
    if (g_host_mallocs++ == g_fail_host_malloc_at) {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    *p = malloc(n ? n : 1);
    g_host.insert(*p);
    return hipSuccess;
}
static hipError_t hipFree(void* p) {
    if (!p) return hipSuccess;
    if (!g_dev.count(p)) violation("hipFree of a block that is not a live device block");
    if (in_flight(p)) violation("hipFree of a device block a queued copy still writes");
    g_dev.erase(p);
    free(p);
    return hipSuccess;
}
static hipError_t hipHostFree(void* p) {
    if (!p) return hipSuccess;
    if (!g_host.count(p)) violation("hipHostFree of a block that is not a live page-locked block");
    if (in_flight(p)) violation("hipHostFree of the page-locked source of a queued copy");
    g_host.erase(p);
    free(p);
    return hipSuccess;
}
static hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    *e = new StubEvent{g_next_event++};
    g_events[(*e)->id] = *e;
    return hipSuccess;
}
static hipError_t hipEventDestroy(hipEvent_t e) {
    if (!e || !g_events.count(e->id)) {
        violation("hipEventDestroy of a dead event");
        return hipErrorInvalidValue;
    }
    g_events.erase(e->id);
    delete e;
    return hipSuccess;
}
static hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    if (!s || !s->alive) return hipErrorInvalidValue;   // a stream the caller has destroyed
    if (g_records++ == g_fail_record_at) return hipErrorInvalidValue;
    if (s->capturing) violation("hipEventRecord on a capturing stream");
    e->recorded = true;
    e->done = false;
    s->pending_events.push_back(e->id);
    return hipSuccess;
}
static hipError_t hipEventQuery(hipEvent_t e) { return !e->recorded || e->done ? hipSuccess : hipErrorNotReady; }
static void drain(hipStream_t s);
static hipError_t hipEventSynchronize(hipEvent_t e) {
    if (e->recorded && !e->done)
        for (StubStream* s : g_streams)
            for (int id : s->pending_events)
                if (id == e->id) {
                    drain(s);
                    return hipSuccess;
                }
    return hipSuccess;
}
static hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t s) {
    if (g_copies++ == g_fail_copy_at) return hipErrorInvalidValue;
    if (!s || !s->alive) return hipErrorInvalidValue;
    if (s->capturing) violation("hipMemcpyAsync on a capturing stream");
    (void)n;
    s->copies.push_back({dst, src});   // the bytes move when the stream is drained
    return hipSuccess;
}
static void drain(hipStream_t s) {
    for (auto& c : s->copies) {
        if (!g_dev.count((void*)c.first)) violation("a queued copy wrote a freed device block");
        if (!g_host.count((void*)c.second) && !g_pageable.count(c.second))
            violation("a queued copy read a freed page-locked block, or a caller's source after the call that took it");
    }
    s->copies.clear();
    for (int id : s->pending_events)
        if (g_events.count(id)) g_events[id]->done = true;
    s->pending_events.clear();
}
static hipStream_t new_stream() {
    g_streams.push_back(new StubStream());
    return g_streams.back();
}
static int g_private_streams = 0;
static hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
    *s = new_stream();
    g_private_streams++;
    return hipSuccess;
}
static hipError_t hipStreamDestroy(hipStream_t s) {
    if (!s->alive) violation("hipStreamDestroy of a dead stream");
    drain(s);
    s->alive = false;
    g_private_streams--;
    return hipSuccess;
}
static hipError_t hipStreamSynchronize(hipStream_t s) {
    if (s->capturing) violation("hipStreamSynchronize of a capturing stream");
    drain(s);
    return hipSuccess;
}
static hipError_t hipStreamIsCapturing(hipStream_t s, hipStreamCaptureStatus* cs) {
    *cs = s && s->capturing ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
    return hipSuccess;
}
static hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
    if (s->capturing) violation("hipStreamWaitEvent on a capturing stream");
    if (!g_events.count(e->id)) violation("hipStreamWaitEvent on a dead event");
    return hipSuccess;
}

#define LZ_CACHE_TEST_STUBS
#include "lanczos_cache.hpp"

static int fails = 0;
#define EXPECT(c)                                         \
    do {                                                  \
        if (!(c)) {                                       \
            printf("FAILED line %d: %s\n", __LINE__, #c); \
            fails++;                                      \
        }                                                 \
    } while (0)

struct Entry {
    int frame, tx, m_b, m_e;
};
struct Key {
    long long k[8];
};
struct Info {
    int n = 0, segs = 1;
    bool balanced = false;
};
typedef lz::UploadCache<Key, Info> Cache;
static const size_t kMaxItems = 64;
static Key make_key(int shape) {
    Key k;
    for (int i = 0; i < 8; i++) k.k[i] = 1000 * i + shape;
    return k;
}
// one insert of `tab`.  An eager upload reads the caller's own (pageable) source, which is only alive during the call
static Cache::Item* put(Cache& c, const Key& k, const std::vector<Entry>& tab, bool balanced, hipStream_t s, hipError_t* e,
                        lz::Upload mode = lz::Upload::on_stream) {
    if (mode == lz::Upload::eager) g_pageable.insert(tab.data());
    Cache::Item* it = c.insert(k, Info{(int)tab.size(), 1, balanced}, tab.data(), sizeof(Entry) * tab.size(), s, mode, e);
    g_pageable.erase(tab.data());
    return it;
}
static bool any_unrecorded(const lz::RetireList& rl) {
    for (auto& r : rl.list)
        if (r.unrecorded) return true;
    return false;
}

int main() {
    hipStream_t s1 = new_stream(), s2 = new_stream();
    {   // 1. a retired block waits for its events; a block whose event could not be recorded waits for the final reap
        lz::RetireList rl;
        void *a, *b, *h;
        hipMalloc(&a, 16), hipMalloc(&b, 16), hipHostMalloc(&h, 16, 0);
        rl.retire({a}, {h}, {s1, s2});
        rl.reap(false);
        EXPECT(g_dev.count(a) && g_host.count(h));          // both events pending
        drain(s1);
        rl.reap(false);
        EXPECT(g_dev.count(a));                             // s2 still pending
        drain(s2);
        rl.reap(false);
        EXPECT(!g_dev.count(a) && !g_host.count(h) && rl.list.empty());
        hipStream_t dead = new_stream();
        dead->alive = false;
        rl.retire({b}, {}, {dead});
        rl.reap(false);
        EXPECT(g_dev.count(b) && rl.list.size() == 1);      // NOT treated as drained
        rl.reap(true);
        EXPECT(!g_dev.count(b) && rl.list.empty());
    }
    EXPECT(g_events.empty());
    {   // 2. the bounded table cache: 200 shapes on a stream that is never drained in between -- evicted tables (device block AND the
        // page-locked source of the upload) must outlive the queued copies; a shape that stays hot is never evicted
        lz::Lifetime life;
        Cache c(&life, kMaxItems);
        const Key hot = make_key(7);
        std::vector<Entry> tab(33, Entry{1, 2, 3, 4});
        hipError_t e = hipSuccess;
        for (int shape = 0; shape < 200; shape++) {
            const Key k = make_key(shape);
            Cache::Item* it = c.find(k);
            EXPECT(it == nullptr || shape == 7);
            if (!it) it = put(c, k, tab, false, shape % 3 ? s1 : s2, &e);
            EXPECT(it && e == hipSuccess && it->n == 33 && it->upload_stream == (shape % 3 ? s1 : s2) && it->streams.size() == 1);
            if (shape >= 7) {
                Cache::Item* h = c.find(hot);     // a hit refreshes the entry
                EXPECT(h != nullptr);
                if (h) lz::note_stream(h->streams, s2);
            }
            EXPECT(c.items.size() <= kMaxItems);
        }
        EXPECT(c.items.size() == kMaxItems && c.find(hot) != nullptr);
        EXPECT(!life.retired.list.empty());                 // nothing was drained: the evicted tables are all still held
        const size_t held = life.retired.list.size();
        EXPECT(held == 200 - kMaxItems);
        drain(s1);
        life.retired.reap(false);
        EXPECT(life.retired.list.size() < held && !life.retired.list.empty());   // the ones uploaded on s2 wait on
        drain(s2);
        life.retired.reap(false);
        EXPECT(life.retired.list.empty());
        // 3. failures inside insert(): nothing leaks, a queued copy's blocks go through the retire list
        Key k = make_key(5000);
        g_fail_host_malloc_at = g_host_mallocs;
        EXPECT(put(c, k, tab, false, s1, &e) == nullptr && e == hipErrorOutOfMemory);
        g_fail_host_malloc_at = -1;
        g_fail_copy_at = g_copies;
        EXPECT(put(c, k, tab, false, s1, &e) == nullptr && e == hipErrorInvalidValue);
        g_fail_copy_at = -1;
        g_fail_record_at = g_records;                       // the copy IS queued, then the record behind it fails
        EXPECT(put(c, k, tab, false, s1, &e) == nullptr && e == hipErrorInvalidValue);
        g_fail_record_at = -1;
        EXPECT(!life.retired.list.empty());                 // both of its blocks wait for s1
        drain(s1);
        life.retired.reap(false);
        EXPECT(c.find(k) == nullptr && life.retired.list.empty());
        // 4. a stream the caller destroys while its tables are cached: eviction cannot record on it and keeps the blocks
        hipStream_t gone = new_stream();
        k = make_key(6000);
        EXPECT(put(c, k, tab, false, gone, &e) != nullptr);
        drain(gone);
        gone->alive = false;
        for (int shape = 7000; shape < 7000 + (int)kMaxItems; shape++) EXPECT(put(c, make_key(shape), tab, false, s1, &e) != nullptr);
        EXPECT(any_unrecorded(life.retired));
        drain(s1);
        life.retired.reap(false);
        EXPECT(any_unrecorded(life.retired));               // still there: only the owner's final reap may free it
        // 5. lanczos_destroy: the device has drained, everything goes, nothing is recorded any more
        drain(s1), drain(s2);
        c.release_all();
        life.release_all();
        EXPECT(c.items.empty() && life.retired.list.empty());
    }
    EXPECT(g_dev.empty() && g_host.empty() && g_events.empty());
    {   // 6. destruction with copies still queued (a context dropped without lanczos_destroy): the destructor waits, then frees
        lz::Lifetime life;
        Cache c(&life, kMaxItems);
        std::vector<Entry> tab(5, Entry{0, 0, 0, 1});
        hipError_t e;
        for (int shape = 0; shape < 3; shape++) EXPECT(put(c, make_key(shape), tab, true, s1, &e) != nullptr);
        c.evict(0);
        drain(s1);   // (release_all's precondition: the owner has drained the device)
    }
    EXPECT(g_dev.empty() && g_host.empty() && g_events.empty());
    {   // 8. first use while the stream is being captured: the table goes up eagerly on the private stream and is complete when
        // insert() returns, nothing is queued on the capturing stream, and eviction keeps the blocks for the live graph
        lz::Lifetime life;
        Cache c(&life, kMaxItems);
        std::vector<Entry> tab(5, Entry{0, 0, 0, 1});
        hipError_t e;
        hipStream_t cap = new_stream();
        cap->capturing = true;
        Cache::Item* it = put(c, make_key(1), tab, true, cap, &e);
        EXPECT(it && e == hipSuccess && it->captured && !it->uploaded && !it->upload_stream && it->streams.empty());
        EXPECT(it && !in_flight(it->dev_block) && life.eager && life.eager != cap && g_private_streams == 1);
        void* dev = it ? it->dev_block : nullptr;
        cap->capturing = false;
        EXPECT(it && c.use(it, s1) == hipSuccess && it->streams.size() == 1);   // eager use: no event to wait for
        it = put(c, make_key(2), tab, true, s1, &e);                            // uploaded on s1, still in flight, then captured
        EXPECT(it && it->uploaded && !it->captured && in_flight(it->dev_block));
        cap->capturing = true;
        EXPECT(it && c.use(it, cap) == hipSuccess && it->captured && !in_flight(it->dev_block) && it->streams.size() == 1);
        cap->capturing = false;
        for (int shape = 100; shape < 100 + (int)kMaxItems; shape++)            // both evicted: kept, not retired
            EXPECT(put(c, make_key(shape), tab, true, s1, &e) != nullptr);
        EXPECT(life.kept_dev.size() == 2 && life.kept_host.size() == 2 && life.retired.list.empty());
        drain(s1);
        life.retired.reap(false);
        EXPECT(g_dev.count(dev));                           // a replay may still read it
        c.release_all();
        life.release_all();
        EXPECT(life.kept_dev.empty() && !life.eager && g_private_streams == 0);
    }
    EXPECT(g_dev.empty() && g_host.empty() && g_events.empty());
    {   // 7. recency order, on the cache itself: a hit moves an entry behind every other, the oldest is the one that goes
        lz::Lifetime life;
        Cache c(&life, 5);
        std::vector<Entry> tab(2, Entry{0, 0, 0, 1});
        hipError_t e;
        for (int i = 0; i < 5; i++) EXPECT(put(c, make_key(i), tab, false, s1, &e) != nullptr);
        EXPECT(c.find(make_key(0)) != nullptr);             // a hit on the oldest
        EXPECT(put(c, make_key(5), tab, false, s1, &e) != nullptr);
        EXPECT(c.peek(make_key(1)) == nullptr && c.peek(make_key(0)) != nullptr);   // 1 went, not 0
        EXPECT(c.find(make_key(2)) != nullptr);
        EXPECT(c.peek(make_key(3)) != nullptr);             // a lookup that does not refresh ...
        EXPECT(put(c, make_key(6), tab, false, s1, &e) != nullptr);
        EXPECT(c.peek(make_key(3)) == nullptr && c.peek(make_key(2)) != nullptr && c.items.size() == 5);   // ... so 3 went
        drain(s1);
    }
    EXPECT(g_dev.empty() && g_host.empty() && g_events.empty());
    {   // 9. a stream that is capturing at eviction: an item used eagerly on a stream that later starts capturing gets no event
        // on it -- the record would become a graph node -- and is not treated as drained
        lz::Lifetime life;
        Cache c(&life, 2);
        std::vector<Entry> tab(2, Entry{0, 0, 0, 1});
        hipError_t e;
        hipStream_t later = new_stream();
        Cache::Item* it = put(c, make_key(0), tab, false, s1, &e);
        EXPECT(it && c.use(it, later) == hipSuccess && it->streams.size() == 2 && !it->captured);
        void* dev = it ? it->dev_block : nullptr;
        drain(s1), drain(later);
        later->capturing = true;
        const int records = g_records;
        EXPECT(put(c, make_key(1), tab, false, s2, &e) && put(c, make_key(2), tab, false, s2, &e));   // evicts shape 0
        EXPECT(g_records == records + 2 + 1);               // the two uploads and s1: nothing on `later`
        EXPECT(life.retired.list.size() == 1 && any_unrecorded(life.retired) && life.kept_dev.empty());
        drain(s1), drain(s2);
        life.retired.reap(false);
        EXPECT(g_dev.count(dev) && life.retired.list.size() == 1);   // every other stream has drained: it stays
        later->capturing = false;
        life.retired.reap(true);
        EXPECT(!g_dev.count(dev) && life.retired.list.empty());
    }
    EXPECT(g_dev.empty() && g_host.empty() && g_events.empty());
    {   // 10. always-eager mode: complete when insert() returns, nothing queued on the caller's stream, no `uploaded` event, no
        // page-locked block; the caller's source may die at once
        lz::Lifetime life;
        Cache c(&life, 4);
        hipError_t e;
        Cache::Item* it;
        const int records = g_records, host_mallocs = g_host_mallocs;
        {
            std::vector<Entry> tab(9, Entry{0, 0, 0, 1});
            it = put(c, make_key(0), tab, false, s1, &e, lz::Upload::eager);
        }
        EXPECT(it && e == hipSuccess && !it->uploaded && !it->upload_stream && !it->host_block && !it->captured && it->streams.empty());
        EXPECT(it && !in_flight(it->dev_block) && s1->copies.empty() && s1->pending_events.empty());
        EXPECT(g_records == records && g_host_mallocs == host_mallocs && life.eager && g_private_streams == 1);
        EXPECT(it && c.use(it, s1) == hipSuccess && c.use(it, s2) == hipSuccess && it->streams.size() == 2);
        std::vector<Entry> tab(9, Entry{0, 0, 0, 1});
        g_fail_copy_at = g_copies;                          // a failed eager insert leaks nothing either
        EXPECT(put(c, make_key(1), tab, false, s1, &e, lz::Upload::eager) == nullptr && e == hipErrorInvalidValue);
        g_fail_copy_at = -1;
        drain(s1), drain(s2);
    }
    EXPECT(g_dev.empty() && g_host.empty() && g_events.empty() && g_private_streams == 0);
    {   // 11. two live items (the resize holds H and V at once) while further inserts run up to and past the bound: neither
        // pointer moves, and the most recently touched item is never the one evicted
        lz::Lifetime life;
        Cache c(&life, 4);
        std::vector<Entry> tab(2, Entry{0, 0, 0, 1});
        hipError_t e;
        for (int round = 0; round < 12; round++) {
            const Key kh = make_key(round % 3), kv = make_key(100 + round);   // H: three shapes in turn, V: always a new one
            Cache::Item* h = c.find(kh);
            if (!h) h = put(c, kh, tab, false, s1, &e, lz::Upload::eager);
            void* const h_block = h ? h->dev_block : nullptr;
            Cache::Item* v = put(c, kv, tab, false, s1, &e, lz::Upload::eager);   // may evict: never h
            EXPECT(h && v && h != v && c.peek(kh) == h && h->dev_block == h_block && g_dev.count(h_block));
            EXPECT(h && memcmp(&h->key, &kh, sizeof(Key)) == 0 && v && c.peek(kv) == v);
            if (h) (void)c.use(h, s1);
            if (v) (void)c.use(v, s1);
            EXPECT(c.items.size() <= 4);
        }
        EXPECT(c.find(make_key(0)) == c.find(make_key(0)));   // a square shape: one entry for both axes
        drain(s1);
    }
    EXPECT(g_dev.empty() && g_host.empty() && g_events.empty());
    {   // 12. one shape captured three times: one item, one device block; evicted, one `kept` entry
        lz::Lifetime life;
        Cache c(&life, 2);
        std::vector<Entry> tab(2, Entry{0, 0, 0, 1});
        hipError_t e;
        hipStream_t cap = new_stream();
        cap->capturing = true;
        const size_t blocks = g_dev.size();
        Cache::Item* first = nullptr;
        for (int i = 0; i < 3; i++) {
            Cache::Item* it = c.find(make_key(0));
            if (!it) it = put(c, make_key(0), tab, false, cap, &e, lz::Upload::eager);
            EXPECT(it && c.use(it, cap) == hipSuccess && it->captured && it->streams.empty());
            if (i == 0) first = it;
            EXPECT(it == first && c.items.size() == 1 && g_dev.size() == blocks + 1);
        }
        cap->capturing = false;
        EXPECT(first && c.use(first, s1) == hipSuccess);    // and once eagerly: it stays a block a graph may name
        EXPECT(put(c, make_key(1), tab, false, s1, &e, lz::Upload::eager) && put(c, make_key(2), tab, false, s1, &e, lz::Upload::eager));
        EXPECT(life.kept_dev.size() == 1 && life.kept_host.empty() && life.retired.list.empty() && g_dev.size() == blocks + 3);
        drain(s1);
    }
    EXPECT(g_dev.empty() && g_host.empty() && g_events.empty());
    {   // 13. the scratch block
        lz::Lifetime life;
        lz::ScratchBlock b;
        hipStream_t cap = new_stream();
        EXPECT(b.reserve(&life, 100, s1, false) == hipSuccess && b.bytes == 100 && b.streams.size() == 1);
        void* p0 = b.p;
        EXPECT(b.reserve(&life, 50, s2, false) == hipSuccess && b.p == p0 && b.bytes == 100 && b.streams.size() == 2);   // never shrinks
        hipEvent_t pending;                                 // (something in flight on s1 when the block is replaced)
        hipEventCreateWithFlags(&pending, 0), hipEventRecord(pending, s1);
        // grown after eager use: the old block is retired on the streams noted on it
        EXPECT(b.reserve(&life, 200, s1, false) == hipSuccess && b.p != p0 && b.bytes == 200 && b.streams.size() == 1);
        EXPECT(life.retired.list.size() == 1 && life.retired.list[0].ev.size() == 2 && !any_unrecorded(life.retired) && g_dev.count(p0));
        drain(s1);
        life.retired.reap(false);
        EXPECT(g_dev.count(p0));                            // s2 has not drained
        drain(s2);
        life.retired.reap(false);
        EXPECT(!g_dev.count(p0) && life.retired.list.empty());
        hipEventDestroy(pending);
        // grown after captured use: a live graph may name the old block: kept
        void* p1 = b.p;
        cap->capturing = true;
        EXPECT(b.reserve(&life, 150, cap, true) == hipSuccess && b.p == p1 && b.captured && b.streams.size() == 1);
        EXPECT(b.reserve(&life, 300, cap, true) == hipSuccess && b.p != p1 && b.captured && b.streams.empty());
        EXPECT(life.kept_dev.size() == 1 && life.kept_dev[0] == p1 && life.retired.list.empty() && g_dev.count(p1));
        cap->capturing = false;
        // grown while a stream noted on it is capturing: no event there, the old block is unrecorded
        lz::ScratchBlock b2;
        EXPECT(b2.reserve(&life, 10, s1, false) == hipSuccess && b2.reserve(&life, 10, cap, false) == hipSuccess && !b2.captured);
        void* p2 = b2.p;
        cap->capturing = true;
        const int records = g_records;
        EXPECT(b2.reserve(&life, 20, s1, false) == hipSuccess && b2.p != p2);
        EXPECT(g_records == records + 1 && life.retired.list.size() == 1 && any_unrecorded(life.retired));
        drain(s1);
        life.retired.reap(false);
        EXPECT(g_dev.count(p2));
        cap->capturing = false;
        // a failed hipMalloc leaves the block empty and usable
        void* p3 = b2.p;
        g_fail_dev_malloc_at = g_dev_mallocs;
        EXPECT(b2.reserve(&life, 40, s1, false) == hipErrorOutOfMemory && !b2.p && b2.bytes == 0 && b2.streams.empty() && !b2.captured);
        g_fail_dev_malloc_at = -1;
        EXPECT(g_dev.count(p3) && life.retired.list.size() == 2);   // the old block went the regular way
        EXPECT(b2.reserve(&life, 40, s1, false) == hipSuccess && b2.p && b2.bytes == 40);
        drain(s1);
    }
    EXPECT(g_dev.empty() && g_host.empty() && g_events.empty());
    for (StubStream* s : g_streams) delete s;
    if (fails || g_violations) {
        printf("cache lifetime: %d failed expectation(s), %d violation(s)\n", fails, g_violations);
        return 1;
    }
    printf("cache lifetime: all cases ok\n");
    return 0;
}
