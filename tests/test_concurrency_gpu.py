"""The library under concurrent streams and host threads.

Every other GPU test makes one call at a time from one host thread.  What exists only for concurrent use is exercised here:

  two streams, one context   a plan or a workgroup table whose upload is still pending on the stream of its first call, used from a
                             second stream (the event wait of UploadCache::use, lanczos_cache.hpp), from a stream that is being captured
                             (the host-side wait: the graph gets no node for the upload), evicted while two streams are in flight
                             (retirement by events on every stream), and context scratch handed from stream to stream by the
                             caller's own events while its block is replaced.  Only the upscale device entry is promised to work
                             from several streams of one context at once; the scratch test orders its streams itself.
  host threads               tests/concurrency_child.py, a fresh process each: concurrent first lanczos_create, the whole job table
                             of tests/concurrency_cfg.py on a context per thread, four threads on one context and one stream through
                             every entry that holds context scratch while a fifth writes the context's settings, contexts closed
                             while others work.  No stream is captured while another thread is inside the library: out of scope.
  the hls::stream adapter    tests/native/compat_threads_check.cpp: lanczos(stream_in, stream_out) from four threads at once.

The filler: torch.cuda._sleep on stream A in front of the first use of a shape, calibrated with events to last between 50 and
500 ms.  It is what makes a two-stream test mean something -- the upload it holds back is still pending when the second stream
asks for the tables -- so every such test asserts `not stream_a.query()` directly after the last call has returned and FAILS
where A had already drained: the path was not exercised.

Expected bytes come from the CPU models (concurrency_cfg.expected) before a second stream or a thread starts; EXACT results are
compared bit for bit, LSB1 results with lsb1_check.check and byte for byte with the same call made alone."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import concurrency_cfg as C
import lanczos_hls_amd as L
import oracle_lib as O
import patterns as P
import resize_filters_model as FM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lanczos-hls_amd")
FILLER_MS = (50.0, 500.0)
NOT_EXERCISED = "stream A had drained before the call on the other stream returned: the pending-upload path was not exercised"


@pytest.fixture(scope="module")
def filler():
    """cycles for torch.cuda._sleep that last 50 .. 500 ms on this device (aimed at 200), measured with events"""
    import torch
    s = torch.cuda.Stream()

    def ms_of(cycles):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    ms_of(1000)                                   # (the kernel's first launch)
    probe = 20_000_000
    cycles = int(probe * 200.0 / max(ms_of(probe), 1e-3))
    ms = ms_of(cycles)
    assert FILLER_MS[0] <= ms <= FILLER_MS[1], f"the filler lasts {ms:.1f} ms, not {FILLER_MS[0]:.0f} .. {FILLER_MS[1]:.0f}"
    print(f"\nfiller: {cycles} cycles = {ms:.1f} ms")
    return cycles


def _fill(stream, cycles):
    import torch
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)


def _single(job, dev):
    """the job once more on a context and a stream of its own, alone: what an LSB1 result must equal byte for byte"""
    import torch
    c = L.Context(0)
    try:
        out = C.device_output(job)
        C.launch(job, c, dev, out, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return C.to_host(job, out)
    finally:
        c.close()


def _check(job, got, what, dev=None, single=None):
    bad = C.output_errors(job, got, what)
    assert not bad, "\n".join(bad)
    if job["check"] == "lsb1":
        single = _single(job, dev) if single is None else single
        assert np.array_equal(got, single), f"{job['name']} {what}: bytes differ from the same call made alone"


# ---- 2. two streams, one context -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["march2-exact", "march3-lsb1", "tile", "ratp", "generic", "hls"])
def test_pending_upload_second_stream(filler, name):
    """The first call of a shape on A behind the filler: the tap tables (and k_march's workgroup table: two events) are queued, not
    up.  The same call on B must wait for them by event and return at once."""
    import torch
    job = C.BY_NAME[name]
    want = C.expected(job)
    dev, y_a, y_b = C.device_inputs(job), C.device_output(job), C.device_output(job)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    ctx = L.Context(0)
    try:
        torch.cuda.synchronize()
        _fill(a, filler)
        C.launch(job, ctx, dev, y_a, a.cuda_stream)
        first = C.report_errors(job, ctx)
        C.launch(job, ctx, dev, y_b, b.cuda_stream)
        busy = not a.query()
        second = C.report_errors(job, ctx)
        tab = ctx.last_march_table()[0]
        torch.cuda.synchronize()
        assert busy, NOT_EXERCISED
        assert not first + second, first + second
        if job["report"]["main"] == C.MARCH:
            assert tab.workgroups > 1, str(tab)
        single = _single(job, dev) if job["check"] == "lsb1" else None
        for tag, y in (("on A", y_a), ("on B", y_b)):
            _check(job, C.to_host(job, y), tag, single=single)
        assert want is C.expected(job)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["march2-exact", "ratp"])
def test_pending_upload_capturing_stream(filler, name):
    """Same start, but B is being captured (relaxed mode): nothing may be waited for ON a capturing stream, so the library waits
    for the upload on the host and the graph gets no node for it.  A second filler behind A's first call keeps A busy beyond that
    wait; an event in front of the first call tells that the wait took place (the first filler is over when the call returns)."""
    import torch
    job = C.BY_NAME[name]
    ins = C.inputs(job)
    dev, y_a, y_b = C.device_inputs(job), C.device_output(job), C.device_output(job)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    before = torch.cuda.Event()
    ctx = L.Context(0)
    g = torch.cuda.CUDAGraph()
    try:
        torch.cuda.synchronize()
        _fill(a, filler)
        before.record(a)
        C.launch(job, ctx, dev, y_a, a.cuda_stream)
        _fill(a, filler)
        with torch.cuda.stream(b):
            g.capture_begin(capture_error_mode="relaxed")
            try:
                C.launch(job, ctx, dev, y_b, b.cuda_stream)
                waited, busy = before.query(), not a.query()
            finally:
                g.capture_end()
        torch.cuda.synchronize()
        assert busy, NOT_EXERCISED
        assert waited, "the captured call returned while the upload was still held back: it did not wait for it on the host"
        assert not C.report_errors(job, ctx)
        _check(job, C.to_host(job, y_a), "eager on A")
        assert int(y_b.max()) == 0, "captured, not run"
        g.replay()
        torch.cuda.synchronize()
        _check(job, C.to_host(job, y_b), "replay")
        # new input data: the graph holds pointers
        other = dict(job, name=job["name"] + "/other", seed=job["seed"] + 500)
        dev["img"].copy_(C.to_device(C.inputs(other)["img"]))
        y_b.zero_()
        g.replay()
        torch.cuda.synchronize()
        _check(other, C.to_host(other, y_b), "second replay, new input")
        assert ins is C.inputs(job)
    finally:
        del g
        ctx.close()


def _shape(i):
    return 64 + 16 * i, 24 + i % 5


def test_eviction_with_two_streams_in_flight(filler):
    """One plan used on A and on B, then 40 more shapes alternately on A and B -- more than the plan cache holds -- with both
    streams held back by fillers: the first plan is evicted while launches that read its tables are queued on two streams, and is
    freed only behind events on both.  One synchronise at the end; the evicted shape is rebuilt; the context closes cleanly."""
    import torch
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    n = 41
    imgs = [P.noise(_shape(i)[1], _shape(i)[0], 3, seed=900 + i) for i in range(n)]
    oracle_of = lambda img: O.expected_hwc_u8(O.cfg(img.shape[1], img.shape[0], 2 * img.shape[1], 2 * img.shape[0], 3, 3, 2, 1), img, 4)
    wants = {i: oracle_of(imgs[i]) for i in (0, 17, 40)}
    descs = [L.make_desc(_shape(i)[0], _shape(i)[1], 3, 2, 1, 3, 1, L.MODE_EXACT) for i in range(n)]
    xs = [torch.from_numpy(img).cuda() for img in imgs]
    new = lambda i: torch.zeros((descs[i].out_h, descs[i].out_w, 3), dtype=torch.uint8, device="cuda")
    ys, y0b, y0again, rerun = [new(i) for i in range(n)], new(0), new(0), [new(i) for i in range(n)]
    ctx, alone = L.Context(0), L.Context(0)
    try:
        torch.cuda.synchronize()
        _fill(a, filler)
        _fill(b, filler)
        ctx.resample_device(descs[0], xs[0].data_ptr(), ys[0].data_ptr(), 1, stream=a.cuda_stream)
        ctx.resample_device(descs[0], xs[0].data_ptr(), y0b.data_ptr(), 1, stream=b.cuda_stream)
        for i in range(1, n):
            ctx.resample_device(descs[i], xs[i].data_ptr(), ys[i].data_ptr(), 1, stream=(b if i % 2 else a).cuda_stream)
            assert ctx.last_route().main == L.ROUTE_MAIN_MARCH, (i, str(ctx.last_route()))
        ctx.resample_device(descs[0], xs[0].data_ptr(), y0again.data_ptr(), 1, stream=a.cuda_stream)   # evicted at the 33rd: rebuilt
        busy = (not a.query(), not b.query())
        torch.cuda.synchronize()
        assert all(busy), f"streams (A, B) still busy after the last call: {busy} -- the plan was not evicted under queued launches"
        st = torch.cuda.current_stream().cuda_stream
        for i in range(n):
            alone.resample_device(descs[i], xs[i].data_ptr(), rerun[i].data_ptr(), 1, stream=st)
        torch.cuda.synchronize()
        for i in range(n):
            got = ys[i].cpu().numpy()
            if i in wants:
                assert np.array_equal(got, wants[i]), f"shape {i} differs from the oracle"
            assert np.array_equal(got, rerun[i].cpu().numpy()), f"shape {i} differs from its single-stream rerun"
        assert np.array_equal(y0b.cpu().numpy(), wants[0]) and np.array_equal(y0again.cpu().numpy(), wants[0])
    finally:
        alone.close()
        assert ctx._h
        ctx.close()      # lanczos_destroy with retired plans pending
        assert not ctx._h


@pytest.mark.parametrize("name", ["march2-exact", "march2-lsb1"])
def test_three_streams_one_plan_interleaved(filler, name):
    """Twelve launches of one shape round-robin over three streams into twelve buffers, the first behind the filler, nothing
    synchronised in between."""
    import torch
    job = C.BY_NAME[name]
    dev = C.device_inputs(job)
    streams = [torch.cuda.Stream() for _ in range(3)]
    ys = [C.device_output(job) for _ in range(12)]
    ctx = L.Context(0)
    try:
        torch.cuda.synchronize()
        _fill(streams[0], filler)
        bad = []
        for k, y in enumerate(ys):
            C.launch(job, ctx, dev, y, streams[k % 3].cuda_stream)
            bad += C.report_errors(job, ctx)
        busy = not streams[0].query()
        torch.cuda.synchronize()
        assert busy, NOT_EXERCISED
        assert not bad, bad
        single = _single(job, dev) if job["check"] == "lsb1" else None
        for k, y in enumerate(ys):
            _check(job, C.to_host(job, y), f"launch {k} on stream {k % 3}", single=single)
    finally:
        ctx.close()


def test_caller_ordered_hand_over_of_scratch(filler):
    """The two-pass intermediate belongs to the context: one stream at a time, the caller orders the streams.  A forced two-pass
    resize on A (behind the filler), B ordered behind A by the caller's event, a larger one on B -- the block is replaced while
    A's launches that use the old one are still queued: retired, not freed --, then A again behind B."""
    import torch
    small, large = C.BY_NAME["two-pass-m"], C.BY_NAME["two-pass-l"]
    assert C.scratch(large)["two-pass"] > C.scratch(small)["two-pass"]
    wants = [C.expected(small), C.expected(large), C.expected(small)]
    dev_s, dev_l = C.device_inputs(small), C.device_inputs(large)
    y1, y2, y3 = C.device_output(small), C.device_output(large), C.device_output(small)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    ctx = L.Context(0)
    try:
        ctx.resize_force(L.RESIZE_TWO_PASS)
        torch.cuda.synchronize()
        _fill(a, filler)
        C.launch(small, ctx, dev_s, y1, a.cuda_stream, set_force=False)
        b.wait_event(a.record_event())
        C.launch(large, ctx, dev_l, y2, b.cuda_stream, set_force=False)
        a.wait_event(b.record_event())
        C.launch(small, ctx, dev_s, y3, a.cuda_stream, set_force=False)
        busy = not a.query()
        assert ctx.last_kernel() == L.KERNEL_RESIZE_TWO_PASS
        torch.cuda.synchronize()
        assert busy, NOT_EXERCISED
        for tag, job, y, want in (("first on A", small, y1, wants[0]), ("larger on B", large, y2, wants[1]), ("again on A", small, y3, wants[2])):
            assert FM.same(C.to_host(job, y), want), f"{tag}: differs from the Pillow model"
    finally:
        ctx.close()


# ---- 3. host threads -----------------------------------------------------------------------------------------------------------
def _child(tmp_path, mode, *args):
    out = str(tmp_path / f"{mode}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LANCZOS_") or k == "LANCZOS_LIB"}
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "concurrency_child.py"), out, mode] + [str(a) for a in args],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"{mode}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    return np.load(out)


def test_threads_with_a_context_and_a_stream_each(tmp_path):
    """a. eight concurrent first lanczos_create; b. every job of the table by eight threads, two passes, thread i from job i // 2
    on, outputs and last_* reports checked by the thread after every call; d. two threads replace their context between the passes
    (lanczos_destroy drains the device under the others).  LSB1 jobs: every thread's bytes equal a single-threaded call's in the
    same process, which meets lsb1_check.check."""
    import concurrency_child as K
    res = _child(tmp_path, "threads")
    assert not res["errors"].size, "\n".join(res["errors"].tolist())
    assert int(res["contexts"]) == K.THREADS == 8
    assert res["calls"].tolist() == [K.PASSES * len(C.TABLE)] * K.THREADS and int(res["jobs"]) == len(C.TABLE)
    starts = [i // 2 for i in range(K.THREADS)]
    assert all(starts.count(s) == 2 for s in set(starts)), "two threads start at each job"


def test_threads_sharing_one_context_and_one_stream(tmp_path, filler):
    """c. four threads walk the scratch-holding entries in ascending scratch size, each from another place, on ONE context and
    ONE stream, every output into a buffer of its own and no device synchronise between the device-entry calls: blocks are
    replaced while earlier launches are queued, and only the context's mutex, held for a whole call, keeps one call's launches
    together.  lanczos_resample_host runs among them (its staging blocks and copy streams are its own); the host entries of the
    resize family use the two-pass intermediate and the converted tensor's bytes from the context's private stream and so, by the
    contract, follow after the one synchronise.  A fifth thread calls force_kernel, resize_force, timing_enable and timing_read
    meanwhile, with settings that change no job's bytes.  No last_* report is asserted: racy by contract on a shared context.
    The filler goes onto the stream before the threads are released, so the calls queue up behind it until something waits for
    the device (a timing_read of a timed launch, the planar entry replacing its frames); the first device call made must have
    found the stream busy, or nothing was queued and the test fails."""
    import concurrency_child as K
    res = _child(tmp_path, "shared", filler)
    assert not res["errors"].size, "\n".join(res["errors"].tolist())
    print(f"\ndevice-entry calls that returned with the stream busy, per thread: {res['busy'].tolist()} of {res['device_calls'].tolist()}")
    assert res["first_busy"].any(), f"first device call of each thread found the stream busy: {res['first_busy'].tolist()} -- " + NOT_EXERCISED
    assert int(res["calls"]) == K.SHARED_THREADS * (len(C.SHARED) + len(C.SHARED_HOST)) and K.SHARED_THREADS == 4
    assert int(res["settings"]) > 0, "the settings thread never ran"
    used = {k for j in C.SHARED + C.SHARED_HOST for k in C.scratch(j)}
    assert used == set(C.SCRATCH_KINDS)


# ---- 4. the adapter ------------------------------------------------------------------------------------------------------------
def test_hls_stream_adapter_from_four_threads(tmp_path):
    """tests/native/compat_threads_check.cpp: lanczos(stream_in, stream_out) of host/hls_compat.hpp, 64 x 48 -> 128 x 96 RGB a = 3,
    from four threads released together (the adapter's context is created by whichever comes first), three calls each on frames
    of their own.  Every output is the oracle's, bit for bit (the adapter runs LANCZOS_MODE_EXACT)."""
    exe, out = str(tmp_path / "compat_threads_check"), str(tmp_path / "compat.bin")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(PKG, "host"),
                    os.path.join(ROOT, "tests", "native", "compat_threads_check.cpp"), "-o", exe, "-L" + PKG, "-llanczos_hip",
                    "-Wl,-rpath," + PKG], check=True, timeout=300)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LANCZOS_")}
    r = subprocess.run([exe, out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out, "rb") as f:
        blob = f.read()
    threads, calls, iw, ih, ow, oh, c, a = struct.unpack_from("<8i", blob)
    assert (threads, calls, iw, ih, ow, oh, c, a) == (4, 3, 64, 48, 128, 96, 3, 3)
    nin, nout, at = iw * ih * c, ow * oh * c, 32
    cfg = O.cfg(iw, ih, ow, oh, c, a, ow // iw, 1)
    seen = set()
    for t in range(threads):
        for k in range(calls):
            img = np.frombuffer(blob, np.uint8, nin, at).reshape(ih, iw, c)
            got = np.frombuffer(blob, np.uint8, nout, at + nin).reshape(oh, ow, c)
            at += nin + nout
            seen.add(img.tobytes())
            assert np.array_equal(got, O.expected_hwc_u8(cfg, np.ascontiguousarray(img), 4)), f"thread {t}, call {k}"
    assert at == len(blob) and len(seen) == threads * calls, "every call had a frame of its own"
