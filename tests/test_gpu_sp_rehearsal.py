"""Multi-rank rehearsal on ONE GPU (2 processes, gloo rendezvous on 127.0.0.1): the kernel-mode model under Ulysses
sequence parallelism and under CFG parallelism must reproduce the single-rank output.  See sp_rehearsal_worker.py."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_on_one_gpu_match_single_rank():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "sp_rehearsal_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"rehearsal failed:\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert r.stdout.count("sp_rel=") == 2, r.stdout[-2000:]
    assert r.stdout.count("fsdp_rel=0.000e+00") == 2, r.stdout[-2000:]  # --dit_fsdp: sharded block weights, bit-equal


def test_two_ranks_ulysses_at_14b_block_dims():
    """Config 4's block dimensions (dim 5120, ffn 13824, 40 heads -> 20 per rank, head-chunked exchange) under pure Ulysses,
    two ranks on the one GPU: bit-equal to the single-rank output."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "sp_rehearsal_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4", WANQ_REHEARSE_DIMS="5120,13824,40,1", WANQ_REHEARSE_NO_CFG_PARALLEL="1")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, f"14B-dims rehearsal failed:\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert r.stdout.count("sp_rel=0.000e+00") == 2, r.stdout[-2000:]
    assert r.stdout.count("fsdp_rel=0.000e+00") == 2, r.stdout[-2000:]


def test_two_ranks_attention_map_quantiser_under_ulysses():
    """attn.attn_map under Ulysses (sp 2): after the head exchange a rank holds all tokens of its heads, so the per-key-column
    statistics over all queries are local -- bit-equal to the single-rank output."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "sp_rehearsal_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4", WANQ_REHEARSE_CONFIG="w8a8_all_linears_attn_map.yaml", WANQ_REHEARSE_NO_CFG_PARALLEL="1")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"attention-map rehearsal failed:\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert r.stdout.count("sp_rel=0.000e+00") == 2, r.stdout[-2000:]



def test_two_ranks_cross_attention_map_quantiser_under_ulysses():
    """cross_attn.attn_map under Ulysses (sp 2): the cross-attention's queries are a token shard, but a key column's step is a maximum
    over ALL queries -- the block gathers the queries of both ranks for it (rank order == sequence order) and keeps its own rows:
    bit-equal to the single-rank output (round 4 refused this combination)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "sp_rehearsal_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4", WANQ_REHEARSE_CONFIG="w8a8_all_linears_attn_map_cross.yaml", WANQ_REHEARSE_NO_CFG_PARALLEL="1")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"cross attention-map rehearsal failed:\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert r.stdout.count("sp_rel=0.000e+00") == 2, r.stdout[-2000:]

def test_two_ranks_int8_qk_under_ulysses():
    """attn.qk under Ulysses (sp 2): q / k are quantised per (token, head) where RMSNorm + RoPE produces them and the head
    exchange moves int8 codes + fp32 scale planes (no silent bf16 path: r2 ADVICE / VERDICT) -- bit-equal to the single-rank
    int8 Q.K^T output; also with cfg-parallel and --dit_fsdp legs of the worker."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "sp_rehearsal_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4", WANQ_REHEARSE_CONFIG="w8a8_all_linears_qk8.yaml", WANQ_REHEARSE_EXPECT_QK8="1")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"int8 Q.K^T rehearsal failed:\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert r.stdout.count("sp_rel=0.000e+00") == 2 and r.stdout.count("qk8_launches_sp=") == 2, r.stdout[-2000:]
    assert r.stdout.count("fsdp_rel=0.000e+00") == 2, r.stdout[-2000:]


def test_two_ranks_fp_model_calibration_and_simulation_mode_under_ulysses():
    """Ulysses for the FP model (fp_generate.py / get_calib_data_wanx.py --ulysses_size P) and for simulation mode
    (quant_generate.py --hardware false): two ranks on the one GPU through the HIP attention kernel against the single-rank run;
    the hooks' per-channel maxima after the MAX all-reduce against the single-rank hooks."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(HERE, "sp_rehearsal_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="4", WANQ_REHEARSE_FP="1")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"FP Ulysses rehearsal failed:\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    assert r.stdout.count("fp_sp_rel=") == 2, r.stdout[-2000:]


@pytest.mark.parametrize("gpus,plan,extra,launcher", [
    (2, "cfg2xsp1", [], "self"),  # `python bench.py --gpus 2`, the form the driver uses at N = 1: bench.py starts its own ranks
    (4, "cfg2xsp2", [], "torchrun"),
    (2, "cfg1xsp2", ["--no-cfg-parallel", "--dit-fsdp", "--quant-config", "w4a8_mixed.yaml"], "torchrun")])
def test_bench_multi_rank_control_flow_rehearsal(gpus, plan, extra, launcher):
    """bench.py --gpus N end to end (cfg-A frame count so that it takes seconds): rendezvous, parallel plan, calibration on
    every rank, timed step with the cfg all-gather, max-over-ranks timing, one JSON line from rank 0 -- under the external
    launcher the driver documents for N > 1, and started bare (no WORLD_SIZE: bench.py launches the ranks as children)."""
    import json

    root = os.path.dirname(HERE)
    args = ["--gpus", str(gpus), "--steps", "1", "--warmup", "0", "--frames", "9", "--full", "--no-cpu-baseline", "--no-quality", *extra]
    if launcher == "self":
        cmd = [sys.executable, os.path.join(root, "bench.py"), *args]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus), "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), os.path.join(root, "bench.py"), *args]
    env = dict(os.environ, OMP_NUM_THREADS="4", WANQ_BENCH_REHEARSE_ON_ONE_GPU="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, f"bench rehearsal failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == gpus and out["config"]["parallelism"] == plan and out["value"] > 0 and out["config"]["rccl_ranks"] == gpus
    assert out["roofline"]["frac"] > 0 and "REHEARSAL" in out["data"]
    # round 5: the HBM-bound kernels and the timed calibration pass ride in the same line (rank 0)
    hb = {r["entry"]: r for r in out["roofline_hbm"]}
    assert {"layernorm_quant", "quant_sum"} <= set(hb) and ({"rmsnorm_rope", "rmsnorm_rope_scatter"} & set(hb))  # (scatter: under Ulysses)
    assert all(0 < r["frac"] < 1 and r["bytes_per_launch"] > 0 for r in hb.values())
    assert out["calibration"]["absmax_launches"] > 0 and out["calibration"]["absmax_TBps"] > 0 and out["calibration"]["ms_per_pass"] > 0
    if extra:  # the flags of BASELINE config 5 (pure Ulysses + sharded packed-W4 / W8 weights), on the 1.3B model
        assert out["config"]["dit_fsdp"]["ranks"] == gpus and "W4A8" in out["config"]["workload"] and "W4A8-mixed" in out["metric"]


def test_bench_single_rank_line_has_every_key_of_the_contract():
    """`python bench.py` at N = 1 on a 9-frame workload (seconds): the driver's contract keys plus `roofline` / `roofline_second_kernel`
    / `roofline_hbm` / `calibration` / `int8_step` / `quality` / `cpu_baseline` (with `cores_available`)."""
    import json

    root = os.path.dirname(HERE)
    env = dict(os.environ, OMP_NUM_THREADS="8")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "WANQ_BENCH_REHEARSE_ON_ONE_GPU"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "1", "--warmup", "1", "--frames", "9", "--full"], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "roofline_second_kernel", "roofline_hbm", "calibration", "int8_step", "quality", "cpu_baseline"):
        assert k in out, k
    assert out["n_gpus"] == 1 and out["steps"] == 1 and out["unit"] == "steps/s" and out["vs_baseline"] is None and out["data"] == "synthetic"
    for ro in (out["roofline"], out["roofline_second_kernel"]):
        assert ro["bound"] == "mfma" and abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-9 and ro["traffic"] is None  # (not the headline workload)
    assert all(abs(h["frac"] - h["TBps"] / 8.0) < 1e-9 for h in out["roofline_hbm"])
    cb = out["cpu_baseline"]
    assert cb["kind"] == "port" and 1 <= cb["cores"] <= cb["cores_available"] and cb["value"] > 0 and cb["cfg_a"]["value"] > 0


def test_bench_plain_line_and_dumped_outputs_match_the_full_run(tmp_path):
    """`python bench.py` without --full carries the headline keys only; --dump-outputs writes the latent of the last timed step, and the
    plain and the --full run (timed calibration pass, instrumented repeat after the dump) dump the same values."""
    import json

    import numpy as np

    root = os.path.dirname(HERE)
    env = dict(os.environ, OMP_NUM_THREADS="8")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "WANQ_BENCH_REHEARSE_ON_ONE_GPU"):
        env.pop(k, None)
    outs = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--no-quality"])):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--frames", "9",
                            "--dump-outputs", str(tmp_path / mode), *extra], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        outs[mode] = json.loads(lines[0])
    plain = outs["plain"]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["steps"] == 2 and abs(plain["value"] * plain["ms_per_step"] - 1e3) < 1e-6
    assert not {"roofline", "roofline_hbm", "calibration", "int8_step", "quality", "cpu_baseline", "instrumented_ms_per_step"} & set(plain)
    assert "roofline" in outs["full"] and "calibration" in outs["full"]
    a, b = np.load(tmp_path / "plain" / "latent.npy"), np.load(tmp_path / "full" / "latent.npy")
    assert a.dtype == np.float32 and a.shape == (16, 3, 60, 104) and np.isfinite(a).all()
    np.testing.assert_array_equal(a, b)


def test_rccl_backend_single_rank_collective_forms():
    """torch.distributed backend "nccl" (= RCCL) itself, world size 1 on the one GPU: the call forms, dtypes and async / side-stream
    semantics of every collective the multi-GPU path issues (rccl_single_rank_worker.py)."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "rccl_single_rank_worker.py"), str(_free_port())],
                       env=dict(os.environ, OMP_NUM_THREADS="4"), capture_output=True, text=True, timeout=300)
    if r.returncode == 3 and "rccl_init_failed" in r.stdout:
        pytest.skip("RCCL could not be initialised on this box: " + r.stdout[-500:])
    assert r.returncode == 0, f"RCCL single-rank worker failed:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert "rccl_single_rank ok=9" in r.stdout, r.stdout[-2000:]
