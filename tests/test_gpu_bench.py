"""GPU tier: bench.py's contract -- one JSON line with the fields the driver reads -- and its
N > 1 code path (gradient accumulation + one RCCL all-reduce per `accum` steps) exercised on one
GPU with a forced one-rank process group."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra_args, env_extra=None):
    env = dict(os.environ)
    env.update(env_extra or {})
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    env["MASTER_PORT"] = str(29850 + os.getpid() % 100)
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "5",
                         "--no-cpu-baseline", "--no-extra"] + extra_args, env=env, cwd=ROOT,
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert pr.returncode == 0, pr.stderr.decode()[-2000:]
    lines = [ln for ln in pr.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, "stdout must carry exactly one line, got %d" % len(lines)
    return json.loads(lines[0])


def _assert_contract_fields(out, steps, warmup):
    assert out["metric"].startswith("queries/sec loss fwd+bwd (B=1024, list_len=128)")
    assert out["n_gpus"] == 1 and out["steps"] == steps and out["warmup"] == warmup
    assert out["unit"] == "queries/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["config"]["mode"] == "eager" and out["config"]["batches_in_rotation"] >= 4
    assert out["value"] > 1e6
    # the timed region is exactly --steps steps, and value and ms_per_step describe the same region
    assert out["config"]["steps_timed"] == steps
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 - 1024) < 1e-6 * 1024


def test_single_gpu_line_has_the_contract_fields():
    out = _run(["--full"])
    _assert_contract_fields(out, 20, 5)
    r = out["roofline"]
    assert r["bound"] == "hbm" and 0 < r["frac"] < 1 and r["peak"] == 8000.0
    assert r["moved_bytes_per_launch"] < r["padded_formula"]["bytes_per_launch"]
    assert abs(r["achieved"] - r["moved_bytes_per_launch"] / (r["kernel_us_avg"] * 1e-6) / 1e9) < 1.0


def test_plain_run_times_the_headline_only_and_dumps_the_last_step(tmp_path):
    """A plain run (no --full) carries the headline fields and none of the separate measurements; --dump-outputs writes
    what the timed region's last step computed, the same from run to run, and that is the fp64 oracle's step on the
    batch that step took, at the weights it started from (the dumped weights + lr * the dumped gradient)."""
    import numpy as np
    outs = []
    for name in ("a", "b"):
        out = _run(["--steps", "7", "--warmup", "3", "--dump-outputs", str(tmp_path / name)])
        _assert_contract_fields(out, 7, 3)
        assert "roofline" not in out and "cpu_baseline" not in out
        assert set(out["extra"]) == {"timed_regions_s", "steps_per_region"}
        outs.append({f[:-4]: np.load(str(tmp_path / name / f)) for f in os.listdir(str(tmp_path / name))})
    a, b = outs
    shapes = {"loss": (1024,), "weight": (136,), "bias": (1,), "grad_weight": (136,), "grad_bias": (1,), "loss_sum": (1,)}
    assert {k: v.shape for k, v in a.items()} == shapes
    for k in shapes:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all(), k
        assert np.allclose(a[k], b[k], rtol=1e-6, atol=1e-7), k
    sys.path.insert(0, ROOT)
    import bench
    from oracle import ltr_oracle as O
    B, L, F, kind = bench.WORKLOADS["c2"]
    last = (7 - 1) % bench.nbuf_for(B, L, F)                  # the timed region's step k takes batch k % nbuf
    _, rel, n, X = bench.synth(B, L, F, last, "cpu")
    W = a["weight"].astype(np.float64) + bench.SGD_LR * a["grad_weight"]
    bias = float(a["bias"][0]) + bench.SGD_LR * float(a["grad_bias"][0])
    want_l, _, want_dW, want_db = O.linear_pairwise(kind, X.numpy(), W, bias, rel.numpy(), n.numpy(), np.full(B, 1.0 / B))
    # (the tolerances of tests/test_gpu_fused.py's _check at this shape)
    assert np.allclose(a["loss"], want_l, rtol=2e-5, atol=1e-5)
    tol = 2e-5 * max(1.0, float(np.max(np.abs(want_dW))))
    assert np.max(np.abs(a["grad_weight"] - want_dW)) < tol
    assert abs(float(a["grad_bias"][0]) - want_db) < tol
    assert np.allclose(a["loss_sum"], want_l.sum(), rtol=1e-4)


def test_forced_process_group_default_is_one_overlapped_allreduce_per_step():
    """The N > 1 headline: one all-reduce per step (north_star / SURVEY.md 8(e)), double-buffered and
    asynchronous; the gradient-accumulation variant rides in extra."""
    out = _run(["--full"], {"LTR_BENCH_FORCE_DIST": "1", "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    assert out["config"]["allreduce_every"] == 1
    assert "one per step" in out["config"]["allreduce"]
    assert out["extra"]["gradient_accumulation_8"]["allreduce_every"] == 8
    assert out["value"] > 1e6


def test_per_step_allreduce_costs_little_more_than_no_allreduce():
    """One rank, RCCL: the step with one all-reduce every step, issued in-stream by the C ABI
    (ltr_linear_step_f32 + RcclOverlap(depth=0)), against the step without any (VERDICT r2 item 4:
    <= 1.15x; a blocking torch.distributed all-reduce per step was 2.3x).  At ONE rank RCCL has nothing to
    exchange, so this bounds the host side of the per-step collective, not its latency over xGMI."""
    env = dict(os.environ)
    env["MASTER_PORT"] = str(29950 + os.getpid() % 40)
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--allreduce-probe"], env=env, cwd=ROOT,
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert pr.returncode == 0, pr.stderr.decode()[-2000:]
    line = [ln for ln in pr.stdout.decode().splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    print(out)
    assert out["raw_rccl_communicator"] and out["raw_rccl_matches_local_step"], out
    assert out["raw_rccl_depth0_us"] <= 1.15 * out["step_without_allreduce_us"] + 1.0, out


def test_forced_process_group_accumulates_and_allreduces():
    out = _run(["--accum", "4"], {"LTR_BENCH_FORCE_DIST": "1", "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    assert out["config"]["allreduce_every"] == 4
    assert out["config"]["steps_timed"] % 4 == 0
    assert out["value"] > 1e6


def test_shard_mode_splits_the_global_batch():
    out = _run(["--workload", "c4", "--shard"])
    assert out["scaling"] == "strong" and out["config"]["global_batch"] == 256


def test_two_ranks_on_one_gpu_run_the_data_parallel_step_with_the_mailbox_allreduce():
    """`bench.py --gpus 2` as the driver launches it, except that both ranks sit on cuda:0 and rendezvous over gloo
    (RCCL refuses two ranks on one device): the whole N > 1 path -- ltr_linear_sgd_step_f32 with the mailbox
    all-reduce between the two processes, the weight update, barrier + max-over-ranks timing, rank 0's JSON line --
    runs for real; only the numbers mean nothing (two processes share one GPU)."""
    port = 29300 + os.getpid() % 300
    procs = []
    for r in range(2):
        env = dict(os.environ)
        env.update({"RANK": str(r), "WORLD_SIZE": "2", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1",
                    "MASTER_PORT": str(port), "LTR_BENCH_BACKEND": "gloo", "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20",
                                       "--warmup", "5", "--no-extra", "--no-cpu-baseline"], env=env, cwd=ROOT,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    outs = []
    for p in procs:
        so, se = p.communicate(timeout=600)
        assert p.returncode == 0, se.decode()[-3000:]
        outs.append(so.decode())
    lines = [ln for ln in outs[0].splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and not [ln for ln in outs[1].splitlines() if ln.startswith("{")]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 2048
    assert "mailbox" in out["config"]["allreduce"], out["config"]["allreduce"]
    assert out["config"]["allreduce_every"] == 1 and out["value"] > 1e5


def test_bare_gpus_2_starts_its_ranks_and_takes_the_one_launch_data_parallel_step():
    """`bench.py --gpus 2` run BARE (no launcher, WORLD_SIZE unset) starts its two ranks itself -- here both
    on cuda:0 over gloo -- and the line says n_gpus 2 with the devices; the step is the data-parallel LAZY one (one launch per
    rank, the all-reduce inside it), the ranks' weights are bit-identical, and the three-launch mailbox step is timed next to it.
    (--workload c2s --shard: two ranks' grids of 256 + 37 workgroups are resident on the one GPU side by side; two C2 grids are
    not, and a launch whose reducers wait for a peer whose launch cannot become resident never ends -- bench.py then takes the
    three-launch mailbox step, which the weak-scaling test above exercises.)"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update({"LTR_BENCH_BACKEND": "gloo", "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "c2s", "--shard", "--steps", "20",
                         "--warmup", "5", "--no-cpu-baseline", "--no-extra", "--full"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                        timeout=600)
    assert pr.returncode == 0, pr.stderr.decode()[-3000:]
    lines = [ln for ln in pr.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and len(out["config"]["devices"]) == 2 and out["scaling"] == "strong"
    dp = out["extra"]["data_parallel"]
    assert dp["weights_bit_identical_across_ranks"] and dp["device_status"] == 0, dp
    assert dp["allreduce_mode"] == "lazy", dp
    assert "ltr_linear_sgd_lazy_step_dp_f32" in out["config"]["allreduce"]
    assert out["extra"]["mailbox_three_launch_step_us"] > 0


def test_world_size_must_match_gpus():
    env = dict(os.environ)
    env.update({"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "5", "--warmup", "1"], env=env,
                        cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert pr.returncode != 0 and b"must agree" in pr.stderr
