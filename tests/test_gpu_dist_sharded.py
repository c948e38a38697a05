"""dist.match_scan_sharded: the whole multi-rank matchScan (round-robin theta shares,
one all-reduce of the record table, index-aware combination) with real kernels.  The
GPU box has one GPU, so the ranks share it and exchange through gloo; with RCCL the
only difference is where the all-reduce runs (bench.py covers that path)."""
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    from ndt_2d_amd import ScanMatcherNDT, synth
    from ndt_2d_amd import dist as shard

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = ScanMatcherNDT(0)
    m.initialize("global_scan_matcher", **synth.matcher_params(1, search_angular_resolution=0.002))
    m.addScans(synth.map_scans(1))
    guess, pts, _ = synth.query_scan(1)
    res = shard.match_scan_sharded(m, guess, pts, rank, world, dist)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), score=res["score"], pose=res["pose"],
             covariance=res["covariance"], best_index=res["best_index"],
             n_candidates=res["n_candidates"])
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_match_scan_equals_single_gpu(tmp_path, world):
    from ndt_2d_amd import ScanMatcherNDT, synth
    ctx = mp.get_context("spawn")
    port = 29600 + world
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    m = ScanMatcherNDT(0)
    m.initialize("single", **synth.matcher_params(1, search_angular_resolution=0.002))
    m.addScans(synth.map_scans(1))
    guess, pts, _ = synth.query_scan(1)
    want = m.matchScan(guess, pts)
    for r in range(world):
        got = np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))
        assert int(got["best_index"]) == want["best_index"]
        assert int(got["n_candidates"]) == want["n_candidates"]
        assert np.array_equal(got["pose"], want["pose"])
        assert abs(float(got["score"]) - want["score"]) < 1e-12
        assert np.allclose(got["covariance"], want["covariance"], rtol=1e-9, atol=0)


def _nccl_worker(out_path):
    """One rank, backend nccl (= RCCL): the collectives of the production path run for
    real -- process group on the GPU, all-reduce of device tensors."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = "29631"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist

    from ndt_2d_amd import ScanMatcherNDT, pf_measure, synth
    from ndt_2d_amd import dist as shard

    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    m = ScanMatcherNDT(0)
    m.initialize("global_scan_matcher", **synth.matcher_params(1))
    m.addScans(synth.map_scans(1))
    guess, pts, _ = synth.query_scan(1)
    res = shard.match_scan_sharded(m, guess, pts, 0, 1, dist)
    # an all-reduce of the record table through RCCL itself (world 1: identity, but the
    # whole code path -- device tensor, RCCL stream hand-off -- runs)
    table = torch.zeros((1, shard.MATCH_RECORD), dtype=torch.float64, device="cuda:0")
    n_th, _, _ = m.prepare_search(guess, pts)
    m.match_launch(0, n_th, record_ptr=table[0].data_ptr())
    m.synchronize()
    dist.all_reduce(table, op=dist.ReduceOp.SUM)
    rec = table.cpu().numpy()[0]
    # sharded particle statistics: the [1, 8] all-reduce on a DEVICE tensor -- the one collective
    # of a step; the theta-variance share stays with the weights (combine_theta_shares)
    parts = synth.particles(3, 4096)
    parts[:, :2] *= 4.0 / 23.0
    d_parts = torch.from_numpy(parts).cuda()
    d_w = torch.zeros(len(parts), dtype=torch.float64, device="cuda:0")
    stats = torch.zeros((1, shard.POSE_STATS), dtype=torch.float64, device="cuda:0")
    m.prepare_beams(pts)
    m.score_poses_launch(d_parts.data_ptr(), len(parts), d_w.data_ptr(), stats[0].data_ptr())
    m.synchronize()
    dist.all_reduce(stats, op=dist.ReduceOp.SUM)
    w, mean, cov, share = shard.finish_particle_statistics(stats.cpu().numpy(), d_w.cpu().numpy(), parts, 0.0)
    cov = shard.combine_theta_shares(cov, [share])
    w1, mean1, cov1 = pf_measure(m, parts, pts)
    np.savez(out_path, score=res["score"], pose=res["pose"], best_index=res["best_index"],
             covariance=res["covariance"], rec=rec, w=w, mean=mean, cov=cov, w1=w1, mean1=mean1, cov1=cov1)
    dist.barrier()
    dist.destroy_process_group()


def test_rccl_single_rank_runs_the_production_collectives(tmp_path):
    """the RCCL path of dist.py (nccl backend: device tensors, no host
    detour) had only ever run under gloo.  One rank is all a 1-GPU box allows."""
    from ndt_2d_amd import ScanMatcherNDT, synth
    out = os.path.join(str(tmp_path), "nccl.npz")
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_nccl_worker, args=(out,))
    p.start()
    p.join(timeout=600)
    assert p.exitcode == 0
    got = np.load(out)
    m = ScanMatcherNDT(0)
    m.initialize("single", **synth.matcher_params(1))
    m.addScans(synth.map_scans(1))
    guess, pts, _ = synth.query_scan(1)
    want = m.matchScan(guess, pts)
    assert int(got["best_index"]) == want["best_index"] == int(got["rec"][1])
    assert np.array_equal(got["pose"], want["pose"])
    assert float(got["score"]) == want["score"]
    assert np.array_equal(got["covariance"], want["covariance"])
    assert np.allclose(got["w"], got["w1"], rtol=1e-12, atol=0)
    assert np.allclose(got["mean"], got["mean1"], rtol=1e-12, atol=1e-15)
    assert np.allclose(got["cov"], got["cov1"], rtol=1e-9, atol=1e-13)


def test_bench_with_eight_ranks_on_one_gpu_finds_the_cfg4_winner(tmp_path):
    """`python bench.py --gpus 8 --full`: bench.py starts the driver's own launch command
    (torch.distributed.run, 8 ranks) as a child process and relays rank 0's line; here
    the ranks share this box's one GPU and exchange through gloo
    (NDT2D_BENCH_BACKEND=gloo): BASELINE.json configs[3] strong-scaled over 8 round-robin
    theta shares must return the oracle's winner over the whole 315.5M-candidate lattice
    (tests/golden/big_winners.json), and configs[4]'s sharded particle statistics must
    agree with the single-process run."""
    import json
    import subprocess
    env = dict(os.environ, NDT2D_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    detail8 = os.path.join(str(tmp_path), "detail8.json")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1",
           "--full", "--detail-file", detail8]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    # stdout: ONE short line (the driver's contract); the full record is in the detail file
    assert len(r.stdout.strip().splitlines()) == 1 and len(r.stdout) < 12288
    short = json.loads(r.stdout)
    with open(detail8) as f:
        line = json.load(f)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "scaling", "dtype"):
        assert short[key] == line[key]
    assert short["roofline"]["frac"] == line["roofline"]["frac"] and short["cpu_baseline"]["value"] > 0
    assert short["particle_filter"]["collectives_per_step"] == 1 and short["detail"]["files"] == [detail8]
    assert len(line["rank_kernel_ms"]["per_rank"]) == 8 and min(line["rank_kernel_ms"]["per_rank"]) > 0
    assert line["speedup_vs_single_gpu_same_workload"] > 0 and line["collective_backend"] == "gloo"
    with open(os.path.join(HERE, "golden", "big_winners.json")) as f:
        want = json.load(f)["cfg4"]
    assert line["n_gpus"] == 8 and line["scaling"] == "strong"
    assert "configs[3]" in line["config"]["workload"]
    assert line["config"]["candidates"] == want["n_candidates"] == 315508257
    assert line["match_result"]["best_index"] == want["best_index"]
    assert [float(v).hex() for v in line["match_result"]["pose"]] == want["pose_hex"]
    assert abs(line["match_result"]["score"] - want["score"]) < 1e-9
    assert line["single_gpu_same_workload"]["ms_per_step"] > 0
    # the N > 1 line counts as measured: a roofline for rank 0's share, the CPU baseline beside it
    assert line["roofline"]["frac"] is not None and 0.0 < line["roofline"]["frac"] <= 1.0
    assert line["roofline"]["valu_insts_per_launch"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["cores"] >= 1
    # ... and the multi-device handle behind the C-ABI found the same winner (8 contexts on this GPU)
    ch = line["c_host_multi_device"]
    assert ch["devices"] == 8 and ch["cfg4"]["best_index"] == want["best_index"]
    assert ch["cfg4"]["variant"].startswith("multi[8]/host/")
    pf = line["particle_filter"]
    assert pf["roofline"]["frac"] is not None and pf["cpu_baseline"]["value"] > 0
    assert "configs[4]" in pf["workload"] and pf["n_gpus"] == 8
    # the same statistics from one process
    env1 = dict(env, NDT2D_BENCH_FORCE_COLLECTIVE="1")
    detail1 = os.path.join(str(tmp_path), "detail1.json")
    r1 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "cfg2", "--steps", "2",
                         "--warmup", "1", "--full", "--no-cpu-baseline", "--no-default-search", "--no-anchors",
                         "--detail-file", detail1],
                        capture_output=True, text=True, timeout=1200, env=env1, cwd=ROOT)
    assert r1.returncode == 0, r1.stderr[-3000:]
    with open(detail1) as f:
        one = json.load(f)["particle_filter_cfg5"]["result"]
    assert pf["result"]["sum_w"] == pytest.approx(one["sum_w"], rel=1e-12)
    assert np.allclose(pf["result"]["mean"], one["mean"], rtol=1e-10, atol=1e-13)
    assert np.allclose(pf["result"]["cov_xx_xy_yy"], one["cov_xx_xy_yy"], rtol=1e-9)
    assert pf["result"]["theta_variance"] == pytest.approx(one["theta_variance"], rel=1e-10)
