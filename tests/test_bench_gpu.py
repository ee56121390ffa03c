"""bench.py's own multi-rank path on the GPU box: `bench.py --gpus 2` with no external launcher
(two ranks spawned by bench.py itself, sharing the one GPU over gloo), checked for the JSON
contract.  8-GPU runs belong to the driver; this is the N > 1 code path at small size."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_self_launches_two_ranks(cuda, tmp_path):
    out = tmp_path / "line.json"
    env = dict(os.environ, LSEC_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "-u", "bench.py", "--gpus", "2", "--stripes", "64", "--steps", "3", "--warmup", "1",
                        "--full", "--no-cpu", "--no-host-path", "--share-gpus", "--json-out", str(out)],
                       cwd=ROOT, env=env, timeout=240, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(out.read_text())
    assert line["n_gpus"] == 2 and line["scaling"] == "weak"
    assert [p["rank"] for p in line["per_rank"]] == [0, 1]
    assert all(p["parity_ok"] and p["stripes"] == 64 for p in line["per_rank"])
    assert line["parity_check"].startswith("bit-exact")
    assert line["value"] > 0 and line["roofline"]["frac"] > 0
    # the one-GPU box: both ranks on one device, and the line says it is a rehearsal
    assert line["distinct_gpus"] == 1 and "rehearsal" in line["config"]["parallelism"]
    assert line["per_rank"][0]["device"]["pci_bus_id"] == line["per_rank"][1]["device"]["pci_bus_id"]
    # the in-run PMC pass runs before the spawn at N > 1 too: traffic on the line
    assert line["roofline"]["traffic"] and "measured in this run" in line["roofline"]["traffic_source"]


@pytest.mark.gpu
def test_bench_refuses_more_ranks_than_gpus(cuda):
    """--gpus 2 on a one-GPU box without --share-gpus is refused before any rank starts"""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "-u", "bench.py", "--gpus", "2", "--stripes", "8", "--no-pmc"], cwd=ROOT, env=env,
                       timeout=120, capture_output=True, text=True)
    assert r.returncode == 2 and "GPU(s) visible" in r.stdout, r.stdout[-1000:] + r.stderr[-1000:]


def test_bench_refuses_mismatched_world_size(tmp_path):
    """(CPU) under an external launcher, WORLD_SIZE must equal --gpus"""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--stripes", "8"], cwd=ROOT, env=env, timeout=120,
                       capture_output=True, text=True)
    assert r.returncode == 2 and "WORLD_SIZE=2" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [None, 3000])
def test_dump_outputs_are_the_last_steps_shards(cuda, tmp_path, monkeypatch, limit):
    """--dump-outputs writes the timed path's parity and rebuilt shards as float32: whole when they
    fit, else the elements a fixed seed picks; the same arguments give the same files, and every
    value written is the reference's (CPU oracle over the same splitmix64 stripes)."""
    import numpy as np

    import bench
    import oracle as O
    from patterns import stripe

    monkeypatch.setenv("LSEC_NUMA", "0")  # leave the test process's CPU affinity alone
    if limit:
        monkeypatch.setattr(bench, "DUMP_ELEMS", limit)
    k, m, C, N = 6, 3, 8192, 5
    got = []
    for d in ("a", "b"):
        a = bench.parse(["--stripes", str(N), "--chunk", str(C), "--steps", "2", "--warmup", "1",
                         "--dump-outputs", str(tmp_path / d)])
        line = bench.run_rank(a, 0, 1, 0)
        assert sorted(line["dump_outputs"]) == ["parity.npy", "rebuilt.npy"] and "roofline" not in line
        got.append({n: np.load(tmp_path / d / n) for n in line["dump_outputs"]})
        assert all(v.dtype == np.float32 for v in got[-1].values())
    for n in got[0]:
        assert np.array_equal(got[0][n], got[1][n])
    data = np.stack([stripe(k, C, s) for s in range(N)])
    want = {"parity.npy": np.stack([O.encode(O.REED_SOL_VAN, data[s], m) for s in range(N)]),
            "rebuilt.npy": data[:, :1]}
    for n, (share, seed) in {"parity.npy": (2, 0x70), "rebuilt.npy": (1, 0x72)}.items():
        ref = want[n].astype(np.float32)
        if limit:
            idx = np.sort(np.random.default_rng(seed).integers(0, ref.size, size=share * limit // 3))
            ref = ref.reshape(-1)[idx]
        assert got[0][n].shape == ref.shape and np.array_equal(got[0][n], ref), n
