"""Multi-process tests of the slab decomposition.
  * CPU (gloo, world_size 2 and 3): communicator primitives, ghost-plane algebra, transposed all-to-all layout.
  * GPU: the slab code path with one rank (local copies) and with 2 / 4 ranks sharing cuda:0 through gloo,
    against the single-GPU path."""
import json
import os
import socket
import tempfile

import numpy as np
import pytest


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(fn, world, *args):
    import torch.multiprocessing as mp
    out = tempfile.mkdtemp()
    mp.spawn(fn, args=(world, _free_port(), out) + args, nprocs=world, join=True)
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_comm_and_halo_gloo_cpu(world):
    from _dist_worker import cpu_comm_worker
    out = _spawn(cpu_comm_worker, world)
    assert all(os.path.exists(os.path.join(out, f"ok_{r}")) for r in range(world))


def _run_bench(extra, env=None):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.pop("RANK", None)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + extra, env=e, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return r, (json.loads(lines[-1]) if lines else None)


@pytest.mark.parametrize("world", [2, 3])
def test_bench_gpus_launches_ranks_cpu(world):
    """`python bench.py --gpus N` with WORLD_SIZE unset starts N rank processes itself (--gpus was ignored):
    the launch / rendezvous / max-over-ranks path rehearsed over gloo on the CPU, no GPU touched."""
    r, line = _run_bench(["--gpus", str(world), "--rehearse"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert line["n_gpus"] == world and line["rccl_world"] == world and line["max_rank_seen"] == world - 1
    # a launcher that disagrees with --gpus is an error, not a silent one-GPU run
    r, line = _run_bench(["--gpus", "2", "--rehearse"], env={"WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0 and line is None and "WORLD_SIZE is 1" in r.stderr


@pytest.mark.gpu
def test_bench_gpus_2_gloo_shared_gpu(gpu):
    """The whole `bench.py --gpus 2 --full` line (slab-decomposed, strong scaling) with two ranks sharing cuda:0 over gloo: a
    rehearsal of the multi-GPU launch, never a measurement."""
    r, line = _run_bench(["--gpus", "2", "--mesh", "64", "--steps", "3", "--warmup", "1", "--n-steps", "3", "--no-cpu-baseline", "--full"],
                         env={"MCPM_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-3000:]
    assert line["n_gpus"] == 2 and line["rccl_world"] == 2 and line["comm_backend"] == "gloo"
    assert line["scaling"] == "strong" and line["value"] > 0 and line["deposits_beyond_ghost_rank0"] == 0
    assert line["config"]["parallelism"] == "slab2"
    ic = line["interleaved_chains"]                      # N > 1: two independent trajectories issued alternately, timed too
    assert ic["chains"] == 2 and ic["value"] > 0 and ic["ms_per_step"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2])
def test_interleaved_chains_equal_solo_runs(gpu, world):
    """Two independent trajectories on their own streams / process groups, issued alternately (`bench.run_interleaved`, the
    multi-chain form that hides one chain's all-to-alls under the other's kernels), reproduce their solo runs bit for bit."""
    from _dist_worker import gpu_interleaved_worker
    out = _spawn(gpu_interleaved_worker, world, 64, 3)
    assert json.load(open(os.path.join(out, "result.json")))["ok"]


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2])
def test_slab_path_against_oracle(gpu, world):
    """BASELINE config 4's workload at test size: the slab-decomposed run (2 ranks over gloo) against the float64
    ORACLE itself (64^3, 3 BullFrog steps, 2LPT start: forward state, density, cell indices, gradient, scalar cotangents),
    with the single-GPU tolerances of test_gpu_golden.py.  The slab FFT needs axes >= 64, so the committed 32^3 fixture
    cannot serve; the oracle vectors are computed here in the layout of tests/golden/nbody_*.npz."""
    from _dist_worker import gpu_slab_golden_worker
    from oracle import pm_oracle as o, background as obg
    from montecosmo_amd import synth
    n, n_steps, a0 = 64, 3, 0.1
    shape = (n, n, n)
    spec = synth.init_mesh(n, seed=11, rms_disp=1.5)
    pos = o.regular_pos(shape)
    cos = obg.Planck18()
    p_o, v_o = o.nbody_bf(cos, spec.astype(np.complex128), pos, a0, 1., n_steps)
    rng = np.random.default_rng(12)
    xb, vb = rng.standard_normal((n ** 3, 3)).astype(np.float32), rng.standard_normal((n ** 3, 3)).astype(np.float32)
    mb_o, sb_o = o.nbody_bf_vjp(cos, spec.astype(np.complex128), pos, xb.astype(np.float64), vb.astype(np.float64), a0, 1., n_steps)
    tmp = os.path.join(tempfile.mkdtemp(), "oracle_64.npz")
    np.savez(tmp, n=n, n_steps=n_steps, a0=a0, init_mesh=spec, final_disp=p_o[0] - pos, final_vel=v_o[0],
             final_cell=o.cell_index(p_o[0], shape), final_density=o.paint(p_o[0], shape), pos_bar=xb, vel_bar=vb,
             init_mesh_bar=mb_o, alpha_bar=sb_o["alpha"], beta_bar=sb_o["beta"],
             lpt_scalar_bars=np.array([sb_o["g"], sb_o["g2"], sb_o["dg2dg"]]))
    out = _spawn(gpu_slab_golden_worker, world, tmp)
    res = json.load(open(os.path.join(out, "result.json")))
    assert res["oob"] == 0
    assert res["disp"] < 1e-5 and res["vel"] < 1e-5 and res["density"] < 1e-5 and res["cell_mismatch"] < 1e-4, res
    assert res["grad"] < 1e-4 and res["alpha"] < 1e-3 and res["beta"] < 1e-3 and res["lpt_scalars"] < 1e-3, res


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [1, 2, 4])
def test_slab_path_single_rank(gpu, chunks):
    """One rank, local-copy communicator: exercises ghost-extended paint/read, the packed (and chunked: every transpose as
    `chunks` all-to-alls of contiguous chunk regions) FFT layouts and the slab adjoint against the plain single-GPU path."""
    from montecosmo_amd import nbody, bricks, synth, dist
    n, n_steps = 64, 3
    shape = (n, n, n)
    spec = synth.init_mesh(n, seed=3, rms_disp=1.5)
    cosmo = bricks.Planck18()
    pm = dist.SlabPM(shape, None, 8, chunks=chunks)
    assert pm.chunks == chunks
    (d, v), ctx = dist.nbody_bf_slab(cosmo, spec, a0=0.1, a1=1.0, n_steps=n_steps, slab=pm, return_ctx=True)
    (lp, v1), c1 = nbody.nbody_bf(cosmo, spec, nbody.LatticePos.regular(shape), a0=0.1, a1=1.0, n_steps=n_steps,
                                  return_ctx=True, lattice_out=True)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    assert rel(d, lp.disp) < 2e-6 and rel(v, v1) < 2e-6
    assert ctx.pm.out_of_ghost() == 0
    rng = np.random.default_rng(5)
    xb = rng.standard_normal((n ** 3, 3)).astype(np.float32)
    vb = rng.standard_normal((n ** 3, 3)).astype(np.float32)
    mb, sb = dist.nbody_bf_slab_vjp(ctx, xb, vb)
    mb1, sb1 = nbody.nbody_bf_vjp(c1, xb, vb)
    assert rel(mb, mb1) < 1e-5
    assert np.allclose(sb["alpha"], sb1["alpha"], rtol=1e-4, atol=1e-4 * np.abs(sb1["alpha"]).max())
    assert np.allclose(sb["beta"], sb1["beta"], rtol=1e-4, atol=1e-4 * np.abs(sb1["beta"]).max())
    for k in ("g", "g2", "dg2dg"):
        assert np.isclose(sb[k], sb1[k], rtol=1e-4, atol=1e-4 * abs(sb1["g"])), k


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_slab_path_multi_rank_shared_gpu(gpu, world):
    from _dist_worker import gpu_slab_worker
    out = _spawn(gpu_slab_worker, world, 64, 3)
    res = json.load(open(os.path.join(out, "result.json")))
    assert res["disp"] < 2e-6 and res["vel"] < 2e-6, res
    assert res["grad"] < 1e-5 and res["alpha"] < 1e-4 and res["beta"] < 1e-4 and res["lpt_scalars"] < 1e-4, res


@pytest.mark.gpu
def test_slab_path_at_the_8_gpu_slab_shape(gpu):
    """256^3 over 4 ranks = local slabs of 64 planes, the per-rank shape of BASELINE config 4 (512^3 over
    8 GPUs), against the single-GPU path (tools/check_slab_large.py as a test; ranks share cuda:0 through gloo).  Forward:
    round-off (measured 8e-8 / 1.5e-7).  Gradient: the two forward states differ by ~1e-7, a few particles sit within that
    distance of a cell face and end in different cells on the two trajectories, and each changes its own gradient row by
    O(1) (profiles/r02_slab_gradient_bisection_128.txt; measured 1.8e-4 here): the bound is DESIGN section 5's."""
    from _dist_worker import gpu_slab_worker
    out = _spawn(gpu_slab_worker, 4, 256, 2)
    res = json.load(open(os.path.join(out, "result.json")))
    assert res["disp"] < 2e-7 and res["vel"] < 4e-7, res
    assert res["grad"] < 1e-3 and res["alpha"] < 2e-3 and res["beta"] < 2e-3 and res["lpt_scalars"] < 2e-3, res


@pytest.mark.gpu
def test_slab_path_at_config4_mesh_size(gpu):
    """BASELINE config 4's MESH (512^3) through the slab path under -m gpu (what's weak 3: it existed only as
    tools/check_slab_large.py): two ranks sharing cuda:0 through gloo, local slabs of 256 planes, against the single-GPU path.  The
    eight-rank split of the same mesh has the slab shape of the test above (64 planes); RCCL with more than one rank cannot run on a
    one-GPU box.  Tolerances as above (measured: forward 1e-7 / 1.7e-7, gradient 8e-5)."""
    from _dist_worker import gpu_slab_worker
    out = _spawn(gpu_slab_worker, 2, 512, 2)
    res = json.load(open(os.path.join(out, "result.json")))
    assert res["disp"] < 2e-7 and res["vel"] < 4e-7, res
    assert res["grad"] < 1e-3 and res["alpha"] < 2e-3 and res["beta"] < 2e-3 and res["lpt_scalars"] < 2e-3, res


@pytest.mark.gpu
def test_predicted_ghost_depth_is_verified(gpu):
    """The exchanged ghost depth of a step is predicted from the previous steps' displacement maxima (no host stop per
    step) and verified one step later: smooth growth stays within the prediction with a spare plane, a jump beyond it is
    reported loudly instead of silently dropping deposits."""
    import torch
    from montecosmo_amd import dist
    pm = dist.SlabPM((32, 32, 32), ghost=8)
    x = torch.zeros((pm.Nl, 3), device="cuda")
    pm.reset_depth()
    used = []
    for amp in (0.4, 0.9, 1.5, 2.2, 3.0):          # displacement maxima of successive steps
        x[:, 0] = amp * torch.sin(torch.arange(pm.Nl, device="cuda") * 0.01)
        pm.set_depth(x)
        used.append(pm.ge)
    pm.finish_depth()
    assert used[0] == 8                            # first step of a trajectory: the full depth
    need = [int(np.floor(a)) + 1 for a in (0.4, 0.9, 1.5, 2.2, 3.0)]
    assert all(u >= n for u, n in zip(used, need)) and used[3] < 8
    pm.reset_depth()
    x[:, 0] = 0.3
    pm.set_depth(x)
    pm.set_depth(x)
    x[:, 0] = 6.5                                  # a jump no smooth trajectory makes
    pm.set_depth(x)
    with pytest.raises(RuntimeError, match="ghost depth"):
        pm.finish_depth()


@pytest.mark.gpu
def test_slab_path_one_rank_rccl(gpu):
    """The communicator's RCCL branch (device tensors in place, asynchronous handles) with the one rank a one-GPU box
    allows: self send/recv for the ghost planes, a one-rank all-to-all for the transposes."""
    from _dist_worker import gpu_slab_worker
    out = _spawn(gpu_slab_worker, 1, 64, 3, "nccl")
    res = json.load(open(os.path.join(out, "result.json")))
    assert res["disp"] < 2e-6 and res["vel"] < 2e-6, res
    assert res["grad"] < 1e-5 and res["alpha"] < 1e-4 and res["beta"] < 1e-4 and res["lpt_scalars"] < 1e-4, res


@pytest.mark.gpu
def test_too_small_ghost_is_detected(gpu):
    """Deposits beyond the ghost planes are counted, so a too-narrow ghost region cannot pass silently."""
    import ctypes as C
    import torch
    from montecosmo_amd import dist
    from montecosmo_amd._lib import POS_LATTICE
    pm = dist.SlabPM((64, 64, 64), ghost=5)
    disp = torch.zeros((pm.Nl, 3), dtype=torch.float32, device="cuda")
    disp[-10:, 0] = 9.5         # last lattice plane, pushed beyond the 5 ghost planes
    disp[:10, 0] = -7.25        # first lattice plane, pushed below them
    pm.call("mcpm_paint_f32", C.c_void_p(disp.data_ptr()), pm.Nl, POS_LATTICE, None, 1, 1.0, 2, C.c_void_p(pm.rho.data_ptr()), 0)
    assert pm.out_of_ghost() == 20
    assert abs(float(pm.rho.double().sum()) - pm.Nl) < 1e-3 * pm.Nl     # mass is clamped, not lost


@pytest.mark.gpu
def test_coherent_flow_beyond_the_ghost_planes_is_counted(gpu):
    """with bulk-centred windows the tile kernels' sure interval reaches |floor(d_x)| = 8 + H, so a COHERENT x flow of
    more than `ghost` cells used to pass the six compares, and its particles beyond the ghost planes were neither listed,
    deposited nor counted.  They must be clamped to the edge plane (mass conserved) and counted."""
    import ctypes as C
    import torch
    from montecosmo_amd import dist
    from montecosmo_amd._lib import POS_LATTICE
    n, G = 64, 8
    pm = dist.SlabPM((n, n, n), ghost=G)
    for flow in (9.3, -9.6):
        before = pm.out_of_ghost()
        disp = torch.zeros((pm.Nl, 3), dtype=torch.float32, device="cuda")
        disp[:, 0] = flow                                  # every particle moves by the same 9+ cells: tile offsets follow it
        disp[:, 1:] = 0.25
        pm.call("mcpm_paint_f32", C.c_void_p(disp.data_ptr()), pm.Nl, POS_LATTICE, None, 1, 1.0, 2, C.c_void_p(pm.rho.data_ptr()), 0)
        oob = pm.out_of_ghost() - before
        # lattice planes whose base cell floor(x + flow) leaves [0, n + 2G - 2] on the ghost-extended mesh
        import math
        planes = sum(1 for x in range(n) if not (0 <= G + x + math.floor(flow) <= n + 2 * G - 2))
        assert planes > 0 and oob == planes * n * n, (flow, oob, planes)
        assert abs(float(pm.rho.double().sum()) - pm.Nl) < 1e-4 * pm.Nl           # clamped, not lost


@pytest.mark.gpu
@pytest.mark.parametrize("world,backend,chunks", [(1, "gloo", 1), (1, "gloo", 2), (1, "gloo", 4), (2, "gloo", None), (4, "gloo", 2),
                                                  (1, "nccl", 2)])
def test_native_slab_steps_equal_the_python_issued_path(gpu, world, backend, chunks):
    """the slab step behind the C ABI (`mcpm_slab_step_f32` / `_vjp_f32`, exchanges issued by the library)
    is bitwise the Python-issued path: one rank with the local transport (1 / 2 / 4 chunks), 2 and 4 gloo ranks through the
    host-callback transport, one RCCL rank on the plan-owned communicator."""
    from _dist_worker import gpu_native_equal_worker
    out = _spawn(gpu_native_equal_worker, world, 64, 3, backend, chunks)
    res = json.load(open(os.path.join(out, "result.json")))
    assert res["ok"], res


@pytest.mark.gpu
def test_failed_transport_self_test_falls_back_on_every_rank(gpu):
    """`mcpm_slab_comm_selftest` runs once after the communicator comes up (an all-to-all, both neighbour exchanges, the max
    all-reduce, verified on the host).  If ONE rank reports a failure, ALL ranks keep the torch.distributed path and the run goes
    on, bitwise equal to a run that asked for that path; `native=True` raises instead.  (What the driver's first multi-GPU run
    would otherwise meet inside its first step.)"""
    from _dist_worker import gpu_native_fallback_worker
    out = _spawn(gpu_native_fallback_worker, 2, 64, 2)
    res = json.load(open(os.path.join(out, "result.json")))
    assert res["ok"], res
    assert "MCPM" in res["reason"] or "rank" in res["reason"], res
