"""Child process of tests/test_concurrency_gpu.py (not collected by pytest): the library from several host threads, in a fresh
process so that its process-wide statics (the launch caches behind launch_cache_mutex(), the environment read once) are cold.

    concurrency_child.py OUT.npz threads    eight threads: concurrent first lanczos_create, then the whole job table of
                                            tests/concurrency_cfg.py twice on a context and a stream per thread -- thread i starts
                                            at job i // 2, so two threads make the process's first launch of each kernel family at
                                            the same moment --, two of them closing their context and creating a new one between
                                            the passes
    concurrency_child.py OUT.npz shared [CYCLES]
                                            four threads on ONE context and ONE stream through the entries that hold context
                                            scratch, a fifth writing the context's settings meanwhile; CYCLES of torch.cuda._sleep
                                            are queued on the stream first, so that the first calls find it busy

The shared library is loaded, the device initialised and every expected array computed in the main thread before a thread starts.
Every thread collects what it finds wrong as text; the process writes the counts and the messages to OUT.npz, prints the messages
and exits with 1 if there are any.  No stream is captured here: capture while another thread is inside the library is outside the
library's contract (a relaxed capture makes the runtime refuse or record other threads' calls) and is not what this tests."""
import os
import sys
import threading
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import concurrency_cfg as C  # noqa: E402
import lanczos_hls_amd as L  # noqa: E402

THREADS, SHARED_THREADS, PASSES = 8, 4, 2
CLOSERS = (1, 6)       # the threads of the per-thread run that replace their context between the passes
BARRIER_S = 60         # a thread that died must not leave the others waiting for ever


def _guard(errors, tag, fn, *a):
    try:
        fn(*a)
    except BaseException:   # noqa: BLE001 -- everything goes into the report
        errors.append(f"{tag}: " + traceback.format_exc(limit=6))


def run_threads(out_path):
    import torch
    L._lib()
    torch.cuda.init()
    jobs = C.TABLE
    for j in jobs:
        C.expected(j)
    dev = {j["name"]: C.device_inputs(j) for j in jobs}
    outs = [{j["name"]: [C.device_output(j) for _ in range(PASSES)] for j in jobs} for _ in range(THREADS)]
    torch.cuda.synchronize()
    errors = [[] for _ in range(THREADS)]
    ctxs = [None] * THREADS
    lsb1 = [dict() for _ in range(THREADS)]    # (job, pass) -> bytes of an LSB1 job, checked by the main thread afterwards
    calls = [0] * THREADS
    start, go = threading.Barrier(THREADS, timeout=BARRIER_S), threading.Barrier(THREADS, timeout=BARRIER_S)

    def worker(i):
        start.wait()
        ctxs[i] = L.Context(0)                 # a. eight first lanczos_create calls at once
        go.wait()
        stream = torch.cuda.Stream()
        for ps in range(PASSES):
            if ps and i in CLOSERS:            # d. lanczos_destroy drains the device while the others work
                ctxs[i].close()
                ctxs[i] = L.Context(0)
            for k in range(len(jobs)):
                job = jobs[(i // 2 + k) % len(jobs)]
                out = outs[i][job["name"]][ps]
                C.launch(job, ctxs[i], dev[job["name"]], out, stream.cuda_stream)
                errors[i] += [f"thread {i} pass {ps}: {e}" for e in C.report_errors(job, ctxs[i])]
                calls[i] += 1
                stream.synchronize()
                got = C.to_host(job, out)
                if job["check"] == "lsb1":
                    lsb1[i][(job["name"], ps)] = got
                else:
                    errors[i] += [f"thread {i} pass {ps}: {e}" for e in C.output_errors(job, got)]

    threads = [threading.Thread(target=_guard, args=(errors[i], f"thread {i}", worker, i)) for i in range(THREADS)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    valid = sum(1 for c in ctxs if c is not None and c._h)
    flat = [e for es in errors for e in es]
    # LSB1: the same call once more, single-threaded, on a context of its own -- every thread's bytes are these, and these meet
    # the contract
    torch.cuda.synchronize()
    one = L.Context(0)
    try:
        for job in jobs:
            if job["check"] != "lsb1":
                continue
            out = C.device_output(job)
            C.launch(job, one, dev[job["name"]], out, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            single = C.to_host(job, out)
            flat += C.report_errors(job, one) + C.output_errors(job, single, "single-threaded")
            for i in range(THREADS):
                for ps in range(PASSES):
                    got = lsb1[i].get((job["name"], ps))
                    if got is None or not np.array_equal(got, single):
                        flat.append(f"thread {i} pass {ps}: {job['name']}: bytes differ from the single-threaded call's")
    finally:
        one.close()
        for c in ctxs:
            if c is not None:
                c.close()
    np.savez(out_path, errors=np.array(flat, dtype=str), contexts=np.array(valid), calls=np.array(calls), jobs=np.array(len(jobs)))
    return flat


def run_shared(out_path, filler_cycles):
    import torch
    L._lib()
    torch.cuda.init()
    order, host_order = C.ascending(C.SHARED), C.ascending(C.SHARED_HOST)
    for j in order + host_order:
        C.expected(j)
    dev = {j["name"]: C.device_inputs(j) for j in order if not j["kind"].startswith("host_")}
    outs = [{j["name"]: C.device_output(j) for j in order if not j["kind"].startswith("host_")} for _ in range(SHARED_THREADS)]
    host_got = [dict() for _ in range(SHARED_THREADS)]
    ctx = L.Context(0)
    ctx.resize_force(C.SHARED_SETTINGS["resize_force"])
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    errors = [[] for _ in range(SHARED_THREADS + 1)]
    done = threading.Event()
    settings = [0]
    busy = [[] for _ in range(SHARED_THREADS)]   # per device-entry call: the stream had work queued when the call returned

    def walk(i, jobs):
        for k in range(len(jobs)):
            job = jobs[(i * len(jobs) // SHARED_THREADS + k) % len(jobs)]   # ascending, each thread from another place
            if job["kind"].startswith("host_"):
                host_got[i][job["name"]] = C.host_call(job, ctx)
            else:
                C.launch(job, ctx, dev[job["name"]], outs[i][job["name"]], stream.cuda_stream, set_force=False)
                busy[i].append(not stream.query())

    def fifth():
        s, n = C.SHARED_SETTINGS, 0
        while not done.is_set():
            ctx.force_kernel(s["force_kernel"][n % 2])
            ctx.timing_enable(s["timing"][n % 2])
            ctx.resize_force(s["resize_force"])
            if n % 4 == 3:
                launches, main_ms, prefix_ms = ctx.timing_read()
                assert launches >= 0 and main_ms >= 0 and prefix_ms >= 0, (launches, main_ms, prefix_ms)
            n += 1
            done.wait(0.0005)
        settings[0] = n

    def phase(jobs):
        go = threading.Barrier(SHARED_THREADS, timeout=BARRIER_S)
        ts = [threading.Thread(target=_guard, args=(errors[i], f"thread {i}", lambda i=i: (go.wait(), walk(i, jobs))))
              for i in range(SHARED_THREADS)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()

    f5 = threading.Thread(target=_guard, args=(errors[SHARED_THREADS], "settings thread", fifth))
    f5.start()
    try:
        if filler_cycles:             # device work in front of everything: the first calls queue up behind it
            with torch.cuda.stream(stream):
                torch.cuda._sleep(filler_cycles)
        phase(order)                  # device entries and lanczos_resample_host: nothing waits for the device in between
        torch.cuda.synchronize()      # the one synchronise
        phase(host_order)             # the host entries of the resize family, on the context's private stream
    finally:
        done.set()
        f5.join()
    flat = [e for es in errors for e in es]
    for i in range(SHARED_THREADS):
        for job in order + host_order:
            if job["kind"].startswith("host_"):
                got = host_got[i].get(job["name"])
                if got is None:
                    flat.append(f"thread {i}: {job['name']}: no result")
                    continue
            else:
                got = C.to_host(job, outs[i][job["name"]])
            flat += [f"thread {i}: {e}" for e in C.output_errors(job, got)]
    ctx.force_kernel(L.KERNEL_NONE)
    ctx.timing_enable(False)
    ctx.resize_force(L.RESIZE_AUTO)
    ctx.close()
    np.savez(out_path, errors=np.array(flat, dtype=str), settings=np.array(settings[0]), first_busy=np.array([b[0] for b in busy]),
             busy=np.array([sum(b) for b in busy]), device_calls=np.array([len(b) for b in busy]),
             calls=np.array(SHARED_THREADS * (len(order) + len(host_order))))
    return flat


if __name__ == "__main__":
    if sys.argv[2] == "threads":
        bad = run_threads(sys.argv[1])
    else:
        bad = run_shared(sys.argv[1], int(sys.argv[3]) if len(sys.argv) > 3 else 0)
    for e in bad[:40]:
        print(e, file=sys.stderr)
    sys.exit(1 if bad else 0)
