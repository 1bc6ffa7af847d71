"""The one call path into libmcpm.so (`_lib.call` / `_lib.marshal`): what it converts, what it passes through and what it rejects
before the library is entered.  Host tests run against the real signature table; the GPU tests issue the same kernels with wrapped
pointers and with tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

from montecosmo_amd import _lib

GROWTH = (0.31, 0.69, 0., -1., 0., -3., 16)      # Omega_m, Omega_de, Omega_k, w0, wa, log10_amin, steps of mcpm_growth_table


def _read_args(pos, mesh, out=None, n=8):
    """mcpm_read_f32(plan = NULL, pos, n, pos_mode, meshes, ncomp, order, out)"""
    return (None, pos, n, _lib.POS_LATTICE, mesh, 1, 2, out)


@pytest.mark.parametrize("name,args,exc,position", [
    ("mcpm_read_f32", _read_args(torch.zeros((8, 3)), None), ValueError, 1),                          # CPU float32 where a device pointer is expected
    ("mcpm_read_f32", _read_args(None, torch.zeros((4, 4, 4), dtype=torch.float64)), TypeError, 4),   # float64 for a float32 kind
    ("mcpm_growth_table", (*GROWTH, *[np.zeros(16, np.float32)] * 7), TypeError, 7),                  # float32 numpy for a host double *
    ("mcpm_growth_table", (*GROWTH, np.zeros(16), np.zeros(32)[::2], *[np.zeros(16)] * 5), ValueError, 8),      # non-contiguous float64 numpy
    ("mcpm_read_f32", _read_args(C.c_void_p(64), torch.zeros((4, 4, 4), dtype=torch.float64)), TypeError, 4),      # ... behind a wrapped pointer
    ("mcpm_read_f32", _read_args(np.zeros((8, 3)), None), TypeError, 1),                              # numpy where a device pointer is expected
    ("mcpm_interp_f32", (None, None, 4, torch.zeros(4), None, 4, 1.0, None), TypeError, 3),           # float32 for a device double *
    ("mcpm_growth_table", (*GROWTH, *[torch.zeros(16, dtype=torch.float64)] * 7), TypeError, 7),      # a tensor for a host double *
])
def test_bad_arguments_are_rejected_with_function_and_position(name, args, exc, position):
    for enter in (lambda: _lib.marshal(name, args), lambda: _lib.call(name, *args)):
        with pytest.raises(exc, match=rf"{name}: argument {position} "):
            enter()


def test_wrong_argument_count_is_a_type_error():
    for args in (_read_args(None, None)[:-1], _read_args(None, None) + (0,)):
        with pytest.raises(TypeError, match=rf"mcpm_read_f32 takes 8 arguments, {len(args)} given"):
            _lib.call("mcpm_read_f32", *args)
    # a tensor, or anything else ctypes refuses, where a number belongs: the same 0-based position as every other message
    for bad, why in ((torch.zeros(1), "is a torch.float32 tensor, expected no array"), ("8", "TypeError")):
        with pytest.raises(TypeError, match=f"mcpm_read_f32: argument 2 {why}"):
            _lib.call("mcpm_read_f32", None, None, bad, 0, None, 1, 2, None)


def test_none_numbers_and_ctypes_objects_pass_through():
    n, p, f = C.c_int64(), C.c_void_p(1 << 20), (C.c_float * 8)()
    for name, args in (("mcpm_plan_last_outliers", (p, C.byref(n))), ("mcpm_read_f32", _read_args(p, None, p)),
                       ("mcpm_bias_weights_f32", (None, 8, p, p, p, p, p, 0, None, 1.0, f, p, p, None))):
        out = _lib.marshal(name, args)
        assert len(out) == len(args) and all(a is b for a, b in zip(out, args)), name
    # None reaches the library as NULL, and its return code goes through `check`
    assert _lib.call("mcpm_plan_destroy", None) is None                       # a NULL plan is accepted: MCPM_OK
    with pytest.raises(_lib.McpmError, match="mcpm_fft_r2c failed with code -6"):
        _lib.call("mcpm_fft_r2c", None, None, None, 1)
    assert _lib.call("mcpm_version").startswith(b"mcpm")                      # not a return code: handed back


def test_numpy_arrays_travel_as_host_doubles():
    """mcpm_growth_table through `call` with arrays and through the library with hand-wrapped pointers: the same tables."""
    a = [np.zeros(16) for _ in range(7)]
    b = [np.zeros(16) for _ in range(7)]
    _lib.call("mcpm_growth_table", *GROWTH, *a)
    assert _lib.lib.mcpm_growth_table(*GROWTH, *[x.ctypes.data_as(C.POINTER(C.c_double)) for x in b]) == 0
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[1][-1] > 0.5


def test_every_signature_has_its_kinds():
    assert set(_lib.KINDS) == set(_lib.SIGNATURES) == set(_lib._CALLS)
    device = 0
    for name, (res, argtypes) in _lib.SIGNATURES.items():
        kinds = _lib.KINDS[name]
        assert len(kinds) == len(argtypes) == len(getattr(_lib.lib, name).argtypes), name
        for k, a in zip(kinds, argtypes):
            assert (k is _lib.HOST_F64) == (a is _lib._f64p), name
            assert bool(k and k is not _lib.HOST_F64) == (a in _lib._DEVICE_DTYPES), name      # device data <=> a tuple of torch dtypes
            device += a in _lib._DEVICE_DTYPES
        assert _lib._CALLS[name][3] == (_lib.VALUE if res is not C.c_int else _lib.PLAN_CODE if argtypes[:1] == [_lib._plan] else _lib.CODE), name
    assert device >= 300      # the table does say what its pointers point at
    assert _lib.KINDS["mcpm_read_f32"][1] == (torch.float32, torch.complex64) and _lib.KINDS["mcpm_cell_index"][5] == (torch.int16,)


def test_context_classes_are_one_class():
    from montecosmo_amd import bricks, dist, model, nbody
    for cls in (bricks.BiasCtx, bricks.PngCtx, bricks.ObsCtx, nbody.LptCtx, nbody.NbodyCtx, dist.SlabCtx, model.EvolveCtx):
        ctx = cls(a=1, b="x")
        assert isinstance(ctx, _lib.Ctx) and (ctx.a, ctx.b) == (1, "x") and getattr(ctx, "missing", None) is None
        assert ctx == ctx and ctx != cls(a=1, b="x") and ctx in {ctx}      # identity, as the separate classes had it
    assert callable(nbody.NbodyCtx.state)


# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tensors_and_wrapped_pointers_give_the_same_bits(gpu):
    """48^3 mesh, 48^3 particles (the smallest mesh the tiled paints accept): paint -> read and the three-component paint on one random
    displacement field, issued with `nbody._ptr` pointers and with the tensors themselves."""
    from montecosmo_amd import nbody
    n = 48
    N = n ** 3
    plan = nbody.get_plan((n, n, n))
    gen = torch.Generator(device=gpu).manual_seed(5)
    disp = (torch.rand((N, 3), device=gpu, generator=gen) - 0.5) * 6.0
    w3 = torch.randn((N, 3), device=gpu, generator=gen)

    def run(p):
        mesh, out = torch.full((n, n, n), torch.nan, device=gpu), torch.full((N,), torch.nan, device=gpu)
        m3 = torch.full((3, n, n, n), torch.nan, device=gpu)
        plan.call("mcpm_paint_f32", p(disp), N, _lib.POS_LATTICE, None, 1, 1.0, 2, p(mesh), 0)
        plan.call("mcpm_read_f32", p(disp), N, _lib.POS_LATTICE, p(mesh), 1, 2, p(out))
        plan.call("mcpm_paint3_f32", p(disp), N, _lib.POS_LATTICE, p(w3), 2, p(m3), 0)
        return mesh, out, m3

    raw, ten = run(nbody._ptr), run(lambda t: t)
    for a, b in zip(raw, ten):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0      # (NaN would compare unequal)
    assert abs(float(raw[0].double().sum()) / N - 1.0) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["column-sliced positions", "float64 mesh", "tensor on another GPU"])
def test_bad_tensors_are_rejected_before_anything_is_enqueued(gpu, case):
    from montecosmo_amd import nbody
    n = 16
    N = n ** 3
    plan = nbody.get_plan((n, n, n))
    pos = torch.zeros((N, 3), device=gpu)
    mesh = torch.ones((n, n, n), device=gpu)
    out = torch.full((N,), -7.0, device=gpu)
    if case == "column-sliced positions":
        pos, exc, where = torch.zeros((N, 4), device=gpu)[:, :3], ValueError, 1
    elif case == "float64 mesh":
        mesh, exc, where = mesh.double(), TypeError, 4
    else:
        if torch.cuda.device_count() < 2:
            pytest.skip("one visible GPU")
        mesh, exc, where = mesh.to("cuda:1"), ValueError, 4
    with pytest.raises(exc, match=rf"mcpm_read_f32: argument {where} "):
        plan.call("mcpm_read_f32", pos, N, _lib.POS_LATTICE, mesh, 1, 2, out)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
