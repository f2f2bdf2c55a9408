"""The prediction of tests/upscale_route_cfg.py tied to a device: a dozen requests of the CPU product, at their tiny sizes, go
through lanczos_resample_device, and the route the call reports (lanczos_last_route) is what predict() says with the facts the
device reports for the instance (lanczos_last_march_table: resident workgroups per CU, CUs).  Together they reach riding, front,
behind, streamed, tile, ratp, rat, generic, a strip without main rows, and a split batch.  Routes only: the bytes of every route
are held by tests/test_upscale_routes_gpu.py."""
import numpy as np
import pytest

import lanczos_hls_amd as L
import upscale_route_cfg as U

pytestmark = pytest.mark.gpu

RGB2X = (1, 3, 2, 3)
K, M_, M2 = U._prefix_rows(2, 3)


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _requests(cus):
    """(name, request, what it was built to reach on a device of `cus` CUs: a (main, prefix) of some launch, or "split")"""
    big = cus + 1   # one prefix workgroup per frame at these widths: more of them than CUs
    return [
        ("riding", U.request(48, M2, 3, 1, 2, 1, 3), (U.MAIN_MARCH, U.PREFIX_RIDING)),
        ("front", U.request(48, M2, 3, 1, 2, 1, 3, frames=big), (U.MAIN_MARCH, U.PREFIX_FRONT)),
        ("behind", U.request(48, M2 - 1, 3, 1, 2, 1, 3, frames=big), (U.MAIN_MARCH, U.PREFIX_BEHIND)),
        ("tile", U.request(46, M2, 3, 1, 2, 1, 3, frames=3), (U.MAIN_TILE, U.PREFIX_BEHIND)),
        ("ratp", U.request(32, 16, 3, 1, 3, 2, 3, frames=3), (U.MAIN_RATP, U.PREFIX_BEHIND)),
        ("rat", U.request(48, 24, 3, 1, 5, 3, 3, frames=3), (U.MAIN_RAT, U.PREFIX_BEHIND)),
        ("generic", U.request(48, M2, 3, 1, 2, 1, 3, frames=3, force=U.KERNEL_GENERIC), (U.MAIN_GENERIC, U.PREFIX_BEHIND)),
        ("generic-5x", U.request(16, 8, 3, 1, 5, 1, 3, frames=2), (U.MAIN_GENERIC, U.PREFIX_BEHIND)),
        ("streamed", U.request(24, 1000, 1, 1, 1, 1, 3, frames=2), (U.MAIN_GENERIC, U.PREFIX_STREAMED)),
        ("main-none", U.request(48, M2 + 4, 3, 1, 2, 1, 3, rows=K, frames=big), (U.MAIN_NONE, U.PREFIX_FRONT)),
        ("below-prefix", U.request(48, M2 + 4, 3, 1, 2, 1, 3, row0=K, rows=4), (U.MAIN_MARCH, U.PREFIX_NONE)),
        ("split", U.request(1040, M2, 3, 1, 2, 1, 3, frames=600), "split"),
        ("hls", U.request(48, 12, 3, 1, 2, 1, 3, mode=U.MODE_HLS, frames=3), (U.MAIN_HLS, U.PREFIX_NONE)),
    ]


def _run(ctx, q):
    import torch
    d = L.make_desc(q.in_w, q.in_h, q.c, q.sn, q.sd, q.a, q.bps, q.mode, q.row0, q.rows)
    in_rows = q.in_h
    if q.rows:
        r0, in_rows = L.strip_input_rows(d, q.row0, q.rows)
    x = torch.randint(0, 256, (q.frames, in_rows * q.in_w * q.c * q.bps), dtype=torch.uint8, device="cuda")
    y = torch.zeros((q.frames, (q.rows or d.out_h) * d.out_w * q.c * q.bps), dtype=torch.uint8, device="cuda")
    ctx.force_kernel(q.force)
    try:
        ctx.resample_device(d, x.data_ptr(), y.data_ptr(), q.frames, 0, 0, torch.cuda.current_stream().cuda_stream)
    finally:
        ctx.force_kernel(L.KERNEL_NONE)
    torch.cuda.synchronize()
    return ctx.last_route(), ctx.last_march_table()


def test_the_device_takes_the_predicted_route(ctx, cus):
    reached, wg_per_cu = set(), {}   # (resident workgroups per CU of an instance: from the first of its calls that marched)
    for name, q, goal in _requests(cus):
        r, (info, _) = _run(ctx, q)
        inst = U.instance(q)
        f = None
        if inst:
            if info.workgroups:
                assert info.cus == cus, f"{name}: {info}"
                wg_per_cu[inst] = info.wg_per_cu
            f = U.facts(inst, wg_per_cu[inst], cus)
        want = U.predict(q, f)
        assert want.err == U.OK, (name, want)
        got = (r.main, r.prefix, set(r.prefix_seen), r.launches)
        assert got == (want.main, want.launches[-1][1], {p for _, p in want.launches}, len(want.launches)), \
            f"{name}: the device reports {r}, predicted {want} with {f}"
        assert (len(want.launches) > 1) if goal == "split" else ((want.main, want.launches[-1][1]) == goal), f"{name}: {want}, built to reach {goal}"
        reached.add(goal)
    assert len(reached) == 12
