"""bench.py as the driver calls it (CPU side): `--gpus N` must never silently run a smaller job, the self-spawn path
starts N ranks, and the N > 1 mode shards ONE image by block rows and gathers the packed blocks on rank 0.  The
multi-rank rehearsal runs with --dry-run (gloo, a stand-in for the encoder: the product has no CPU path)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["MASTER_ADDR"] = "127.0.0.1"
    env.update(kw)
    return env


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_gpus_2_without_gpus_fails_loudly():
    import pytest
    if not _no_gpu():
        pytest.skip("a GPU is present")
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"], env=_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "GPU" in p.stderr
    assert '"n_gpus"' not in p.stdout  # no line that could be mistaken for a result


def test_world_size_mismatch_is_refused():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--dry-run"], env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "WORLD_SIZE" in p.stderr and '"n_gpus"' not in p.stdout


def test_one_gpu_without_gpu_fails_loudly():
    import pytest
    if not _no_gpu():
        pytest.skip("a GPU is present")
    p = subprocess.run([sys.executable, BENCH, "--steps", "1", "--warmup", "0", "--no-cpu", "--no-extra"], env=_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and '"value"' not in p.stdout


def test_self_spawn_two_ranks_dry_run():
    """python bench.py --gpus 2 (no launcher): two gloo ranks, one image sharded by block rows, gather on rank 0"""
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run", "--size", "256", "--steps", "3", "--warmup", "1"],
                       env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1  # rank 0 only
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["dry_run"] is True and r["value"] is None
    assert r["scaling"] == "strong" and r["steps"] == 3 and r["warmup"] == 1
    assert r["config"]["blocks_per_rank"] == [2048, 2048]
    assert "gather" in r["config"]["exchange"] and "rank 0" in r["config"]["exchange"]
    assert "BASELINE configs[4]" in r["config"]["workload"]
    assert r["output_check"]["matches_single_process"] is True
    assert r["output_check"]["steps_checked"] == 3 and r["output_check"]["every_step_identical"] is True


def test_three_ranks_ragged_shards_dry_run():
    """64 block rows over 3 ranks: 21 / 21 / 22 rows, no padding, same gathered image"""
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
                        "--master-port", "29741", BENCH, "--gpus", "3", "--dry-run", "--size", "256", "--steps", "2", "--warmup", "0"],
                       env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert r["n_gpus"] == 3 and r["config"]["blocks_per_rank"] == [21 * 64, 21 * 64, 22 * 64]
    assert r["output_check"]["matches_single_process"] is True


def test_dump_outputs_dry_run(tmp_path):
    """--dump-outputs DIR: the blocks of the last timed step as float32 DIR/bc7_blocks.npy, byte for byte what the stand-in
    computes on the whole image, and the same file for two runs with the same arguments"""
    sys.path.insert(0, ROOT)
    import bench
    import numpy as np
    import torch
    from convectionkernels_amd import synth
    want = bench.stand_in_encoder(torch.from_numpy(synth.tile_blocks(synth.image_rgba8(5, 256, 256)))).numpy()
    for k in range(2):
        d = tmp_path / str(k)
        p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--dry-run", "--size", "256", "--steps", "2", "--warmup", "1",
                            "--dump-outputs", str(d)], env=_env(), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        assert r["steps"] == 2 and "ms_per_step" in r
        got = np.load(d / "bc7_blocks.npy")
        assert got.dtype == np.float32 and got.shape == (4096, 16)
        assert (got == want).all()


def test_dump_outputs_samples_rows_beyond_the_limit(tmp_path, monkeypatch):
    """an output larger than DUMP_LIMIT_BYTES as float32 is cut to a fixed, seeded sample of whole rows in block order"""
    sys.path.insert(0, ROOT)
    import bench
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100 * 16 * 4)
    blocks = np.arange(1000 * 16, dtype=np.uint32).reshape(1000, 16)
    blocks = (blocks % 251).astype(np.uint8)
    blocks[:, 0] = np.arange(1000) % 256
    blocks[:, 1] = np.arange(1000) // 256
    dumps = []
    for k in range(2):
        bench.dump_outputs(str(tmp_path / str(k)), blocks)
        dumps.append(np.load(tmp_path / str(k) / "bc7_blocks.npy"))
    a = dumps[0]
    assert a.dtype == np.float32 and a.shape == (100, 16) and a.nbytes <= bench.DUMP_LIMIT_BYTES
    assert (a == dumps[1]).all()
    idx = (a[:, 0] + 256 * a[:, 1]).astype(np.int64)
    assert (np.diff(idx) > 0).all() and (a == blocks[idx]).all()


def test_roofline_arithmetic_on_synthetic_counters():
    """bench.roofline_block: VALU issue fraction, HBM view and traffic ratio from given counters (no profile, no GPU)"""
    sys.path.insert(0, ROOT)
    import bench
    # 1116 wave-instructions per block, 1 Mi blocks in 1.55 ms -> 0.61 of the 1.2288e12 wave-inst/s issue peak
    r = bench.roofline_block("bc7", 1 << 20, 1.55, "k", insts_per_block=1116.0, hbm_bytes_per_block=81.5)
    assert r["bound"] == "valu" and abs(r["frac"] - 1116.0 * (1 << 20) / 1.55e-3 / 1.2288e12) < 1e-6
    assert abs(r["traffic_over_algorithmic"] - 81.5 / bench.ALGO_BYTES["bc7"]) < 1e-9 and r["hbm"]["frac"] < 0.01
    assert bench.roofline_block("bc1", 4096, 0.04, "k")["bound"] == "hbm"  # no counters: the HBM view alone, with a note


def test_committed_profiles_feed_the_rooflines_when_they_belong_to_this_library():
    """The counters bench.py quotes (VALU instructions per block, HBM bytes per launch) come from profiles/rNN/*.json and are
    used only for the library they were taken with: the build identity compiled into the library (a hash of the kernel / shim
    sources, public headers and compiler flags, csrc/Makefile) must equal the one the newest committed summaries carry --
    otherwise bench.py marks them `stale` and reports the HBM view alone.  A stale profile is a to-do for whoever holds an
    MI355X (tools/profile_round.sh + tools/profile_formats.sh + tools/install_profiles.sh), not a failure of the CPU suite."""
    import glob
    import json
    sys.path.insert(0, ROOT)
    import bench
    from convectionkernels_amd import api
    sha = api.library_source_sha256()
    assert len(sha) == 64
    summaries = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "summary.json")))
    assert summaries
    head = json.load(open(summaries[-1]))
    if head["source_sha256"] != sha:
        pmc = bench.profiled_counters(sha)
        assert pmc is None or pmc.get("stale")  # never quoted as if they were this library's
        pytest.skip("profiles/ were taken with another build of the library (%s...): re-profile on an MI355X" % head["source_sha256"][:12])
    pmc = bench.profiled_counters(sha)
    assert pmc and not pmc.get("stale") and pmc["blocks"] == 1 << 20
    r = bench.roofline_block("bc7", pmc["blocks"], 1.55, "k", insts_per_block=pmc["valu_insts_per_wave"] / 16.0,
                             hbm_bytes_per_block=pmc["hbm_bytes_per_launch"] / float(pmc["blocks"]))
    assert r["bound"] == "valu" and 0.3 < r["frac"] < 1.0 and 0.99 < r["traffic_over_algorithmic"] < 1.2 and r["hbm"]["frac"] < 0.01
    fmtc = bench.format_counters(sha)
    assert fmtc and not fmtc.get("stale")
    for fmt in ("bc7", "bc7o", "bc7u", "bc6hu", "etc2rgba", "bc1"):
        c = fmtc[fmt]
        assert c["valu_wave_insts_per_block"] > 100 and c["hbm_bytes_per_block"] > 64, (fmt, c)
    # BC6H keeps its search state on the chip: traffic ~ algorithmic (round 3: 687 x)
    assert fmtc["bc6hu"]["hbm_bytes_per_block"] < 1.2 * bench.ALGO_BYTES["bc6hu"]


def test_the_printed_line_stays_short_enough_for_the_driver():
    """Round 5's single line had grown to 21 KB and the driver's parser gave up on it (BENCH_r05.parsed = null).  The line
    is now a summary (bench.compact_line) and every leg in full goes to bench_detail.json: on the largest result there is --
    round 5's full N = 1 result, every leg present, plus padding in every free-text field -- it stays under 4 KB and still
    carries the contract's fields, `roofline` and `cpu_baseline`."""
    sys.path.insert(0, ROOT)
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r05", "bench.json")))
    full["config"]["workload"] = full["config"]["workload"] + " (padding)" * 5
    full["cpu_baseline"]["sample"] = "x" * 2000
    full["roofline"]["note"] = "y" * 2000
    full["output_check"] = {"matches_reference": True, "steps_checked": 20, "every_step_identical": True, "sha256": "0" * 64}
    line = bench.compact_line(full)
    assert len(line) < 4096 and "\n" not in line
    r = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"):
        assert k in r, k
    assert r["config"]["workload"].startswith("EncodeBC7")
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms"):
        assert k in r["roofline"], k
    assert set(("achieved", "peak", "frac", "traffic_over_algorithmic")) <= set(r["roofline"]["hbm"])
    for k in ("value", "unit", "cores", "kind", "sample", "gpu_mismatching_blocks", "blocks_checked"):
        assert k in r["cpu_baseline"], k
    assert r["cpu_baseline"]["one_thread"]["value"] > 0 and r["bit_exact_vs_cpu"] is True
    assert set(r["configs"]) == set(full["configs"]) and all("sha_ok" in v for v in r["configs"].values())
    # a result with fifty more configs drops the optional parts instead of growing past the limit
    for i in range(50):
        full["configs"]["extra_%d" % i] = full["configs"]["3_bc6hu_4096"]
    line = bench.compact_line(full)
    assert len(line) < 4096 and "roofline" in json.loads(line) and "cpu_baseline" in json.loads(line)
