"""bench.py's multi-GPU launcher: `--gpus N` without a torch.distributed
environment starts N rank processes itself, before anything touches a GPU, and the JSON line
reports the initialised world.  CPU: --dry-run (gloo ranks, no GPU work).  GPU: two product
ranks sharing GPU 0 through the launch path (one MI355X per box; the service grid needs the
whole GPU, so ranks that share one run the launch path)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, timeout=300):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [2, 3, 8])
def test_dry_run_launches_n_ranks(n):
    d = _bench("--dry-run", "--gpus", str(n), "--n", "100", "--steps", "3", "--warmup", "1")
    assert d["n_gpus"] == n
    assert len(d["per_rank_ms"]) == n
    assert d["backend"] == "gloo"


def test_dry_run_single_rank_does_not_spawn():
    d = _bench("--dry-run", "--steps", "2")
    assert d["n_gpus"] == 1 and len(d["per_rank_ms"]) == 1


@pytest.mark.gpu
def test_two_product_ranks_on_one_gpu():
    """Two ranks, each verifying its own resident records with the HIP kernels (launch path),
    every bitmap checked against the generator truth inside bench.py.  The line reports the
    one physical GPU and the two ranks separately."""
    d = _bench("--full", "--gpus", "2", "--same-device", "--launch-only", "--n", "65536", "--rotate", "2", "--steps", "4",
               "--warmup", "2", "--no-extras", "--no-host-e2e", "--cpu-budget", "0", timeout=600)
    assert d["n_gpus"] == 1 and d["ranks"] == 2 and d["same_device"]["ranks"] == 2
    assert len(d["per_rank_ms"]["all"]) == 2
    assert d["value"] > 0 and d["roofline"]["kernel"].startswith("k_verify_batches (one batch per launch")


@pytest.mark.gpu
def test_two_batch_list_ranks_on_one_gpu():
    """The default headline (one hfv_verify_batches launch per K steps) with two ranks on GPU 0:
    each rank's launches use the whole chip and share it with the other's; every bitmap is
    checked against the generator truth inside bench.py; the line reports both ranks."""
    d = _bench("--full", "--gpus", "2", "--same-device", "--n", "262144", "--rotate", "2", "--steps", "8", "--warmup", "2",
               "--no-extras", "--no-host-e2e", "--cpu-budget", "0", timeout=600)
    assert d["n_gpus"] == 1 and d["ranks"] == 2 and len(d["per_rank_ms"]["all"]) == 2
    assert d["roofline"]["kernel"] == "k_verify_batches" and d["value"] > 0
    assert d["batches"]["kernel_ms"] > 0


@pytest.mark.gpu
def test_two_service_ranks_on_one_gpu():
    """the service path with two ranks on GPU 0, each resident grid limited to
    half the CUs (hfv_service_set_grid: CUs / ranks), both timed together; every bitmap is checked
    against the generator truth inside bench.py, and each rank reports its thread budget."""
    d = _bench("--full", "--gpus", "2", "--same-device", "--n", "262144", "--rotate", "2", "--steps", "8", "--warmup", "2",
               "--no-extras", "--no-host-e2e", "--cpu-budget", "0.2", "--mode", "service", timeout=600)
    assert d["n_gpus"] == 1 and d["ranks"] == 2 and len(d["per_rank_ms"]["all"]) == 2
    # the N > 1 line carries its CPU baseline (rank 0, after every rank's GPU legs)
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] >= 1 and cb["verdicts_match_gpu"] is True, cb
    assert d["roofline"]["kernel"] == "k_verify_service" and d["value"] > 0
    assert int(d["same_device"]["service_grid_blocks"]) * 2 <= 256
    assert d["host_threads"]["ranks_on_node"] == 2 and d["host_threads"]["budget"] >= 1   # OMP_NUM_THREADS=1 here
    # per-rank grid times.  Each rank's grid verifies 8 x 2^18 records on half the
    # CUs side by side with the other's: about as long as one full-chip grid over 8 x 2^19
    # (~0.1 ms at 0.7 of 8 TB/s); neither rank's grid runs at the pace of host round trips (the
    # round-3 fault: ~40 us per batch; block_waits == 0 below is the deterministic check) and the
    # two stay within 2.5x of each other (timing bounds loose: ADVICE r04).
    g = d["per_rank_ms"]["grid_ms"]
    assert len(g) == 2 and all(0 < x < 1.0 for x in g), g
    assert max(g) < 2.5 * min(g), g
    assert all(r["block_waits"] == 0 for r in d["service"]["relay"]), d["service"]["relay"]


@pytest.mark.gpu
def test_two_loop_ranks_on_one_gpu():
    """config 5 (hfv_loop_run: producer threads -> RX ring -> router kernel ->
    TX/drop consumers) with two ranks at once, the way the driver's N > 1 run executes it (every
    rank runs the loop leg; here both on GPU 0).  Per rank: rx/tx/drop/byte/verdict counts and the
    order-free digest of every transmitted (rewritten) frame equal the oracle router's over the
    same cyclic frame sequence, and every producer and consumer thread ended its work on a CPU of
    the GPU's NUMA node.  The headline (batch-list) and service legs ran first on both ranks."""
    import numpy as np
    from scion_hfv import evaluation as E
    from test_gpu_loop import _oracle
    total = 300_000
    d = _bench("--full", "--gpus", "2", "--same-device", "--n", "65536", "--rotate", "2", "--steps", "4", "--warmup", "2",
               "--no-host-e2e", "--cpu-budget", "0", "--big-n", "0", "--br-n", "0", "--loop-n", str(total),
               "--loop-chunk", "16384", "--loop-chunks", "6", "--loop-threads", "3", "--loop-consumers", "2",
               "--loop-digest", timeout=900)
    assert d["n_gpus"] == 1 and d["ranks"] == 2
    loop = d["config5_loop"]
    assert "error" not in loop, loop
    want = _oracle(E.frames(1000), total)
    per = loop["per_rank"]
    assert [p["rank"] for p in per] == [0, 1]
    for p in per:
        assert p["error"] is None, p
        for k in ("rx", "tx", "tx_bytes", "drop", "verdicts"):
            assert p[k] == want[k], (p["rank"], k, p[k], want[k])
        assert int(p["tx_digest"], 16) == want["tx_digest"], p["rank"]
        assert p["threads"] >= 2
        if p["numa_node"] >= 0:
            assert p["threads_on_node"] == p["threads"], p
    assert loop["mpkts"] > 0 and np.isfinite(loop["mpkts"])


@pytest.mark.gpu
def test_single_rank_line_keeps_the_contract():
    """The driver's N = 1 line: every contract key, `value` = whole-job Mpkt/s over the timed
    steps, the roofline and cpu_baseline objects (bench contract, task 4), and the per-grid
    clock and balance-weight diagnostics of the service regions."""
    d = _bench("--full", "--steps", "6", "--warmup", "2", "--no-extras", "--no-host-e2e", "--loop-n", "0", "--cpu-budget", "1",
               timeout=600)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["unit"] == "Mpkt/s" and d["dtype"] == "u8" and "workload" in d["config"]
    assert abs(d["value"] - 2 ** 20 / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 0.01
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and 0 < r["frac"] < 1
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    c = d["cpu_baseline"]
    assert c["value"] > 0 and c["cores"] >= 1 and c["kind"] in ("reference", "port") and c["sample"]
    s = d["service"]
    assert len(s["grids_mhz"]) == len(s["grids_ms"]) and all(len(w) == 9 for w in s["weights"])


PLAIN_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config")
FULL_ONLY = ("roofline", "cpu_baseline", "service", "batches", "per_launch", "stream_read", "ceilings", "config3",
             "config4", "config5_loop", "host_e2e", "pcie_probe", "sustained", "per_call", "mall_resident",
             "hbm_resident")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["batches", "service", "launch"])
def test_plain_run_times_the_headline_alone_and_dumps_its_last_step(mode, tmp_path):
    """A plain run (no --full): the contract fields with `value` = Mpkt/s over the K timed steps of
    the chosen path, none of the --full legs in the line, and --dump-outputs holding the last timed
    step's verdicts (step K - 1 verifies resident batch (K - 1) % R): one float32 0/1 per record,
    equal to the generator truth of that batch, ragged last word included."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    n, R, K = 65536 + 37, 3, 8
    d = _bench("--steps", str(K), "--warmup", "2", "--n", str(n), "--rotate", str(R), "--mode", mode,
               "--dump-outputs", str(tmp_path / "out"))
    for k in PLAIN_KEYS:
        assert k in d, k
    assert not [k for k in FULL_ONLY if k in d]
    assert d["n_gpus"] == 1 and d["steps"] == K and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["unit"] == "Mpkt/s" and d["dtype"] == "u8" and d["metric"] == bench.METRIC
    assert d["value"] > 0 and abs(d["value"] - n / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 0.01
    assert os.listdir(tmp_path / "out") == ["verdicts.npy"]
    v = np.load(tmp_path / "out" / "verdicts.npy")
    assert v.dtype == np.float32 and v.shape == (n,)
    assert np.array_equal(v != 0, ~bench.corrupted(n, ((K - 1) % R) * n))
    assert set(np.unique(v)) <= {0.0, 1.0}


def test_dump_sample_is_fixed_and_within_the_cap():
    """--dump-outputs keeps a larger output as a sample: the same sorted, distinct rows in every
    run, and no more than the cap allows; an output under the cap is kept whole."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.dump_sample(1 << 20, 12, 1.0) is None
    a, b = bench.dump_sample(1 << 24, 12, 1.0), bench.dump_sample(1 << 24, 12, 1.0)
    assert (a == b).all() and (a[1:] > a[:-1]).all() and 0 <= a[0] and a[-1] < 1 << 24
    assert len(a) * 12 <= bench.DUMP_CAP_BYTES < (len(a) + 1) * 12
