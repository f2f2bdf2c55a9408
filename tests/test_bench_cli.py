"""bench.py plumbing.  On any machine (children that need no GPU see none): `--gpus N` starts its own ranks (a child
torch.distributed.run) before the process touches the GPU, a rank without a GPU refuses to run (no CPU fallback), the option
checks, and what --dump-outputs writes.
On the GPU (marked): a plain run times exactly K steps, prints the headline line only, and dumps the last step's output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env_without_gpus():
    """The environment of a child that sees no GPU on any machine (device list "-1": no visible device), no rank variables."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    return env


def test_bench_refuses_without_a_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1"], capture_output=True, text=True,
                       timeout=300, env=_env_without_gpus())
    assert r.returncode != 0 and "needs a GPU" in (r.stderr + r.stdout)


def test_bench_gpus_n_launches_its_own_ranks():
    """No RANK/WORLD_SIZE in the environment: the parent must spawn 2 ranks; with no GPU visible both fail ("needs a
    GPU"), which shows they were started with rank environments, and the parent passes the failure code on."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"],
                       capture_output=True, text=True, timeout=600, env=_env_without_gpus())
    assert r.returncode != 0
    assert (r.stderr + r.stdout).count("needs a GPU") >= 2


def test_csrc_fingerprint_is_stable():
    sys.path.insert(0, ROOT)
    import bench
    a, b = bench.csrc_fingerprint(), bench.csrc_fingerprint()
    assert a == b and len(a) == 16


def test_side_measurement_options_need_full():
    for opt in ("--planar-path", "--exchange"):
        r = subprocess.run([sys.executable, BENCH, opt], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "add --full" in r.stderr
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_dump_outputs_is_a_fixed_float32_sample_within_budget(tmp_path, monkeypatch):
    """dump_outputs on a host tensor: the head rows of frame 0 and the seeded sample, as float32 sample values (uint16
    carried in int16 comes out unsigned), the same on every call, no more than DUMP_SAMPLES in all."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLES", 300_000)

    class Wl:
        pass

    g = torch.Generator().manual_seed(5)
    for hi, dt in ((256, torch.uint8), (65536, torch.int16)):
        wl = Wl()
        wl.y = torch.randint(0, hi, (4, 300, 400, 3), generator=g, dtype=torch.int32).to(dt)
        want = wl.y.to(torch.int32).numpy() & (hi - 1)
        got = []
        for run in range(2):
            d = tmp_path / f"{hi}_{run}"
            bench.dump_outputs(torch, wl, str(d), 0, 1)
            assert sorted(os.listdir(d)) == ["output_head.npy", "output_sample.npy"]
            head, sample = np.load(d / "output_head.npy"), np.load(d / "output_sample.npy")
            assert head.dtype == sample.dtype == np.float32
            assert head.size + sample.size <= 300_000 and sample.size > head.size > 0
            assert head.shape == (300_000 // 3 // 1200, 400, 3) and np.array_equal(head, want[0, :head.shape[0]])
            idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, want.size, size=sample.size))
            assert np.array_equal(sample, want.reshape(-1)[idx]) and sample.max() >= hi // 2
            got.append((head, sample))
        assert all(np.array_equal(a, b) for a, b in zip(got[0], got[1]))


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_the_last_step(tmp_path):
    """A plain run prints the headline fields and none of --full's side measurements, with `steps` = K timed steps in one
    region; --dump-outputs writes the last timed step's output, identical on a second run, and equal (within the default
    mode's 1 LSB) to the CPU checker on the input set that step read."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    import oracle_lib as O

    K, W = 7, 3
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, BENCH, "--config", "c1", "--steps", str(K), "--warmup", str(W),
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["value"] > 0 and line["ms_per_step"] > 0
        assert line["steps"] == K and line["timing"]["regions"] == 1 and line["timing"]["steps_per_region"] == K
        assert not {"roofline", "cpu_baseline", "other_patterns", "other_configs", "host_path_pinned"} & set(line)
        dumps.append({n: np.load(d / n) for n in sorted(os.listdir(d))})
    assert sorted(dumps[0]) == ["output_head.npy", "output_sample.npy"]
    assert sum(a.nbytes for a in dumps[0].values()) <= 64e6
    for n in dumps[0]:
        assert dumps[0][n].dtype == np.float32 and np.array_equal(dumps[0][n], dumps[1][n]), n

    iw, ih, c, bps, sn, sd, a, _ = bench.CONFIGS["c1"]
    s = (W + K - 1) % line["config"]["batch_sets_cycled"]
    frame = bench.make_frames(torch, "gradient", line["config"]["frames_per_step_per_gpu"], ih, iw, c, bps,
                              torch.device("cuda", 0), 1234 + 1000 * s)[0].cpu().numpy()
    want = O.expected_hwc_u8(O.cfg(iw, ih, iw * sn // sd, ih * sn // sd, c, a, sn, sd), frame, 8).astype(np.float32)
    head = dumps[0]["output_head.npy"]
    assert np.abs(head - want[:head.shape[0]]).max() <= 1
