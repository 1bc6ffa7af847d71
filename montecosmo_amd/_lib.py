"""ctypes binding of libmcpm.so (the C ABI declared in include/mcpm.h).

The HIP library is the product: there is NO CPU fallback.  Importing this module without a built
`libmcpm.so` next to it raises ImportError with the build command.
"""
import ctypes as C
import os
import re
import types

import numpy as np
import torch  # must be imported first: libmcpm.so binds to the HIP runtime / rocFFT torch loaded

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MCPM_LIB") or os.path.join(_HERE, "libmcpm.so")      # MCPM_LIB: another build of the same ABI (A/B runs on one box)

OK = 0
POS_ABSOLUTE, POS_LATTICE = 0, 1
AP_NONE, AP_AUTO, AP_PARAM = 0, 1, 2
LIK_SHASH, LIK_POISSON, LIK_TWO_QUAD = 0, 1, 2
FD_INF, FD_2, FD_4 = 0, 2, 4


# What a pointer argument points at.  Device pointers travel as integers (to ctypes each kind is a c_void_p); `call` takes a tensor
# there and checks it against the kind.  A plain C.c_void_p is an opaque handle (stream, communicator id, callbacks).
def _kind(name, doc):
    return type(name, (C.c_void_p,), {"__doc__": doc})


_plan = _kind("_plan", "mcpm_plan *: the handle whose error text `check` reads")
_f32p = _kind("_f32p", "device float *: float32 data, or complex64 (half-spectra travel as float pairs)")
_d64p = _kind("_d64p", "device double *: tables, reduction outputs")
_i16p = _kind("_i16p", "device int16_t *")
_u32p = _kind("_u32p", "device unsigned *: torch keeps such slots as int32")
_u8p = _kind("_u8p", "device bytes: bool masks, untyped uint8 workspace")
_realp = _kind("_realp", "device const void *: float32 or float64 data, told apart by a flag of the call")
_f64p = C.POINTER(C.c_double)      # host double *: `call` takes a float64 numpy array there
_DEVICE_DTYPES = {_f32p: (torch.float32, torch.complex64), _d64p: (torch.float64,), _i16p: (torch.int16,),
                  _u32p: (torch.int32, torch.uint32), _u8p: (torch.uint8, torch.bool), _realp: (torch.float32, torch.float64)}
HOST_F64 = "host float64"

# name -> (restype, argtypes); mirrors include/mcpm.h one to one
SIGNATURES = {
    "mcpm_plan_create": (C.c_int, [C.c_int] * 6 + [C.c_void_p, C.POINTER(C.c_void_p)]),
    "mcpm_plan_create_slab": (C.c_int, [C.c_int] * 6 + [C.c_void_p, C.POINTER(C.c_void_p)]),
    "mcpm_plan_slab_oob": (C.c_int, [_plan, C.POINTER(C.c_int64)]),
    "mcpm_plan_destroy": (C.c_int, [_plan]),
    "mcpm_last_error": (C.c_char_p, [_plan]),
    "mcpm_version": (C.c_char_p, []),
    "mcpm_plan_last_outliers": (C.c_int, [_plan, C.POINTER(C.c_int64)]),
    "mcpm_plan_last_bucketed": (C.c_int, [_plan, C.POINTER(C.c_int64)]),
    "mcpm_plan_last_paint_stats": (C.c_int, [_plan, C.POINTER(C.c_int64)]),
    "mcpm_plan_set_centre": (C.c_int, [_plan, C.c_int]),
    "mcpm_plan_set_lattice_patch": (C.c_int, [_plan, C.c_int]),
    "mcpm_plan_chained_fb": (C.c_int, [_plan, C.c_double, C.c_double, _f32p, _f32p, C.POINTER(C.c_void_p)]),
    "mcpm_plan_set_halo": (C.c_int, [_plan, C.c_int]),
    "mcpm_plan_set_paint3_fixed": (C.c_int, [_plan, C.c_int]),
    "mcpm_plan_last_redo": (C.c_int, [_plan, C.POINTER(C.c_int64)]),
    "mcpm_fft_r2c": (C.c_int, [_plan, _f32p, _f32p, C.c_int]),
    "mcpm_fft_c2r": (C.c_int, [_plan, _f32p, _f32p, C.c_int]),
    "mcpm_cell_index": (C.c_int, [_plan, _f32p, C.c_int64, C.c_int, C.c_int, _i16p]),
    "mcpm_paint_f32": (C.c_int, [_plan, _f32p, C.c_int64, C.c_int, _f32p, C.c_int64, C.c_float, C.c_int, _f32p, C.c_int]),
    "mcpm_paint_kb_f32": (C.c_int, [_plan, _f32p, C.c_int64, C.c_int, _f32p, C.c_int64, C.c_float, C.c_int, C.c_float, _f32p, C.c_int]),
    "mcpm_read_kb_f32": (C.c_int, [_plan, _f32p, C.c_int64, C.c_int, _f32p, C.c_int, C.c_float, _f32p, _f32p, C.c_int64, C.c_float, _f32p]),
    "mcpm_paint3_f32": (C.c_int, [_plan, _f32p, C.c_int64, C.c_int, _f32p, C.c_int, _f32p, C.c_int]),
    "mcpm_paint3_scaled_f32": (C.c_int, [_plan, _f32p, C.c_int64, C.c_int, _f32p, C.c_float, C.c_int, _f32p, C.c_int]),
    "mcpm_read_f32": (C.c_int, [_plan, _f32p, C.c_int64, C.c_int, _f32p, C.c_int, C.c_int, _f32p]),
    "mcpm_paint_vjp_f32": (C.c_int, [_plan, _f32p, C.c_int64, C.c_int, _f32p, C.c_int64, C.c_float, C.c_int, _f32p, _f32p, _f32p]),
    "mcpm_read_vjp_pos_f32": (C.c_int, [_plan, _f32p, C.c_int64, C.c_int, _f32p, C.c_int, C.c_int, _f32p, _f32p]),
    "mcpm_kspace_force_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_float, C.c_int, C.c_int, C.c_float, C.c_int]),
    "mcpm_kspace_force_vjp_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_float, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mcpm_kspace_hessian_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_float, C.c_int, C.c_int]),
    "mcpm_kspace_hessian_vjp_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mcpm_kspace_phase_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mcpm_hessian_combine_f32": (C.c_int, [_plan, _f32p, _f32p]),
    "mcpm_hessian_combine_vjp_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p]),
    "mcpm_force_meshes_f32": (C.c_int, [_plan, _f32p, _f32p]),
    "mcpm_force_meshes_vjp_f32": (C.c_int, [_plan, _f32p, _f32p]),
    "mcpm_bias_fields_f32": (C.c_int, [_plan, _f32p, C.c_float, C.c_float, C.c_float, _f32p]),
    "mcpm_bias_fields_vjp_f32": (C.c_int, [_plan, _f32p, C.c_float, C.c_float, C.c_float, _f32p, _f32p]),
    "mcpm_bias_fields_save_f32": (C.c_int, [_plan, _f32p, C.c_float, C.c_float, C.c_float, _f32p, _f32p]),
    "mcpm_bias_fields_vjp_saved_f32": (C.c_int, [_plan, C.c_float, C.c_float, C.c_float, _f32p, _f32p, _f32p]),
    "mcpm_bias_weights_f32": (C.c_int, [_plan, C.c_int64, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_int64, _f32p, C.c_float,
                                        C.POINTER(C.c_float), _f32p, _f32p, _d64p]),
    "mcpm_bias_weights_vjp_f32": (C.c_int, [_plan, C.c_int64, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_int64, _f32p, C.c_float,
                                            C.POINTER(C.c_float), _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _d64p]),
    "mcpm_eulerian_bias_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float), _f32p, _f32p, _d64p]),
    "mcpm_eulerian_bias_vjp_f32": (C.c_int, [_plan, _f32p, _d64p, C.c_int, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float), _f32p, _f32p,
                                            _f32p, _d64p]),
    "mcpm_power_mult_f32": (C.c_int, [_plan, _f32p, C.c_float, C.c_float, C.c_float, C.c_double, _d64p, _d64p, C.c_int, _f32p]),
    "mcpm_interp_f32": (C.c_int, [_plan, _f32p, C.c_int64, _d64p, _d64p, C.c_int, C.c_float, _f32p]),
    "mcpm_png_add_f32": (C.c_int, [_plan, _f32p, C.c_float, C.c_float, C.c_float, _d64p, _d64p, C.c_int, C.c_float, C.c_int, _f32p,
                                   _f32p, _d64p]),
    "mcpm_png_add_vjp_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, _d64p, C.c_float, C.c_float, C.c_float, _d64p, _d64p,
                                       C.c_int, C.c_float, _f32p, _f32p, _f32p, _f32p, _d64p, _d64p]),
    "mcpm_png_phi_f32": (C.c_int, [_plan, _f32p, C.c_float, C.c_float, C.c_float, _d64p, _d64p, C.c_int, _f32p, _f32p]),
    "mcpm_png_div_f32": (C.c_int, [_plan, _f32p, C.c_float, C.c_float, C.c_float, _d64p, _d64p, C.c_int, C.c_float, _f32p]),
    "mcpm_png_weights_f32": (C.c_int, [_plan, C.c_int64, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_float, C.POINTER(C.c_float), _f32p, _d64p]),
    "mcpm_png_weights_vjp_f32": (C.c_int, [_plan, C.c_int64, _f32p, _f32p, _f32p, _f32p, _f32p, C.c_float, C.POINTER(C.c_float), _f32p,
                                           _f32p, _f32p, _f32p, _f32p, _f32p, _d64p]),
    "mcpm_kaiser_post_c64": (C.c_int, [_plan, _f32p, _f32p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_double, _d64p, _d64p, C.c_int]
                                      + [C.c_double] * 10 + [_f32p, _f32p, _f32p]),
    "mcpm_kaiser_sky_f32": (C.c_int, [_plan, _f32p, _f32p, _f64p, C.c_int, _d64p, C.c_int, C.c_int] + [C.c_double] * 4 + [_f32p]),
    "mcpm_kaiser_sky_vjp_f32": (C.c_int, [_plan, _f32p, _f32p, _f64p, C.c_int, _d64p, C.c_int, C.c_int] + [C.c_double] * 4
                                         + [_f32p, _f32p, _f32p, _d64p]),
    "mcpm_kaiser_sky_tables_vjp_f32": (C.c_int, [_plan, _f32p, _f64p, C.c_int, _d64p, C.c_int, C.c_int, C.c_double, _f32p, _d64p]),
    "mcpm_lik_real_f32": (C.c_int, [_plan, C.c_int, C.c_int64, _f32p, _f32p, _f32p, C.c_float, _u8p, C.c_float, C.c_float, C.c_float,
                                    _f32p, _f32p, _d64p]),
    "mcpm_lik_real_phi_f32": (C.c_int, [_plan, C.c_int, C.c_int64, _f32p, _f32p, _f32p, C.c_float, _u8p, _f32p] + [C.c_float] * 5
                                       + [_d64p, _d64p, C.c_int, _f32p, _f32p, _f32p, _d64p]),
    "mcpm_lik_fourier_f32": (C.c_int, [_plan, _f32p, _f32p] + [C.c_float] * 10 + [_f32p, _d64p]),
    "mcpm_lik_fourier_temp_f32": (C.c_int, [_plan, _f32p, _f32p] + [C.c_float] * 11 + [_f32p, _d64p]),
    "mcpm_lpt_combine_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, C.c_int64, _f32p, _f32p]),
    "mcpm_lpt_combine_vjp_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, C.c_int64, _f32p, _f32p, _f32p]),
    "mcpm_observe_pos_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_int,
                                       _d64p, C.c_int, C.c_int, _f32p]),
    "mcpm_observe_pos_vjp_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_int,
                                           _d64p, C.c_int, C.c_int, _f32p, _f32p, _f32p, _f32p, _d64p]),
    "mcpm_lightcone_tables_vjp_f32": (C.c_int, [_plan, _f32p, C.c_int64, _d64p, C.c_int, C.c_int, _f32p, _f32p, _f32p, _d64p]),
    "mcpm_observe_pos_tables_vjp_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_int,
                                                  _d64p, C.c_int, C.c_int, _f32p, _d64p]),
    "mcpm_observe_pos_ap_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_int,
                                          _d64p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _d64p, C.c_int, C.c_int, _f32p]),
    "mcpm_observe_pos_ap_vjp_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_int,
                                              _d64p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _d64p, C.c_int, C.c_int,
                                              _f32p, _f32p, _f32p, _f32p, _d64p, _d64p]),
    "mcpm_observe_pos_ap_tables_vjp_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_int,
                                                     _d64p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _d64p, C.c_int,
                                                     C.c_int, _f32p, _d64p]),
    "mcpm_rg2cgh_f32": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, _f32p]),
    "mcpm_rg2cgh_vjp_f32": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, _f32p]),
    "mcpm_cgh2rg_f32": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, _f32p]),
    "mcpm_cgh2rg_amp_f32": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, _f32p]),
    "mcpm_chreshape_c64": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, _f32p, C.c_int, C.c_int, C.c_int]),
    "mcpm_chreshape_vjp_c64": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, _f32p, C.c_int, C.c_int, C.c_int]),
    "mcpm_slab_spec_elems": (C.c_int64, [_plan]),
    "mcpm_slab_zfwd": (C.c_int, [_plan, _f32p, C.c_int64, _f32p, C.c_int]),
    "mcpm_slab_ycol": (C.c_int, [_plan, _f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mcpm_slab_ycol2": (C.c_int, [_plan, _f32p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mcpm_slab_set_window": (C.c_int, [_plan, C.c_int, C.c_int]),
    "mcpm_slab_set_chunks": (C.c_int, [_plan, C.c_int]),
    "mcpm_slab_xfused": (C.c_int, [_plan, _f32p, _f32p, C.c_int]),
    "mcpm_slab_zinv": (C.c_int, [_plan, _f32p, _f32p, C.c_int64, C.c_int]),
    "mcpm_pm_forces_f32": (C.c_int, [_plan, _f32p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _f32p]),
    "mcpm_pm_forces_spec_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, _f32p]),
    "mcpm_pm_forces_vjp_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_int64, C.c_int, C.c_int, _f32p, _f32p, _f32p]),
    "mcpm_pm_forces2_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _f32p]),
    "mcpm_plan_force_meshes": (C.c_int, [_plan, C.POINTER(C.c_void_p)]),
    "mcpm_drift_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_int64, C.c_float, _f32p]),
    "mcpm_kick_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_int64, C.c_float, C.c_float, _f32p]),
    "mcpm_kick_drift_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_int64, C.c_int, _f32p, C.c_int, C.c_float, C.c_float, C.c_float, _f32p, _f32p]),
    "mcpm_kick_drift_il_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_int64, C.c_int, _f32p, C.c_int, C.c_float, C.c_float, C.c_float, _f32p, _f32p]),
    "mcpm_plan_track_dmax": (C.c_int, [_plan, _u32p]),
    "mcpm_slab_zinv3_il": (C.c_int, [_plan, _f32p, _f32p]),
    "mcpm_plan_profile": (C.c_int, [_plan, C.c_int]),
    "mcpm_plan_profile_read": (C.c_int, [_plan, C.c_int, _f64p, _f64p, C.POINTER(C.c_int64)]),
    "mcpm_stage_name": (C.c_char_p, [C.c_int]),
    "mcpm_bullfrog_step_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_double, C.c_double, C.c_double, C.c_int, _f32p, _f32p, _f32p]),
    "mcpm_bullfrog_step_vjp_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, C.c_double, C.c_double, C.c_double, C.c_int, _f32p, _f32p, _d64p, _d64p, C.c_double, _d64p]),
    "mcpm_bullfrog_step_vjp_from_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, C.c_double, C.c_double, C.c_double, C.c_int, _f32p, _f32p, _f32p, _f32p, _d64p, _d64p, C.c_double, _d64p]),
    "mcpm_plan_hint_next_adjoint": (C.c_int, [_plan, C.c_double, C.c_double]),
    "mcpm_step_adjoint_particles_il_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, _f32p, C.c_double, C.c_double, C.c_double, C.c_int, _f32p, _f32p, _d64p, _d64p, C.c_double, _d64p]),
    "mcpm_step_adjoint_particles_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, _f32p, C.c_double, C.c_double, C.c_double, C.c_int, _f32p, _f32p, _d64p, _d64p, C.c_double, _d64p]),
    "mcpm_lpt_accum_f32": (C.c_int, [_plan, _f32p, C.c_float, C.c_float, C.c_int, _f32p, _f32p]),
    "mcpm_lattice_scatter_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_float, C.c_float, _f32p]),
    "mcpm_lattice_dot_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, _d64p]),
    "mcpm_lpt_vjp_opts_f32": (C.c_int, [_plan, _f32p, C.c_int, _f64p, C.c_int, C.c_int, _f32p, _f32p, _f32p, _f64p]),
    "mcpm_pm_forces_vjp_opts_f32": (C.c_int, [_plan, _f32p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _f32p]),
    "mcpm_lpt_vjp_f32": (C.c_int, [_plan, _f32p, C.c_int, _f64p, _f32p, _f32p, _f32p, _f64p]),
    "mcpm_lpt_f32": (C.c_int, [_plan, _f32p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, _f32p, _f32p]),
    "mcpm_lpt_save_f32": (C.c_int, [_plan, _f32p, C.c_int, C.c_float, C.c_float, C.c_float, _f32p, _f32p, _f32p]),
    "mcpm_lpt_vjp_saved_f32": (C.c_int, [_plan, _f32p, C.c_int, _f64p, _f32p, _f32p, _f32p, _f32p, _f64p]),
    "mcpm_nbody_bf_f32": (C.c_int, [_plan, _f32p, C.c_int, _f64p, _f64p, C.c_double, _f64p, C.c_int, C.c_int, _f32p, _f32p, _f32p]),
    "mcpm_nbody_ckpt_floats": (C.c_int64, [_plan, C.c_int, C.c_int]),
    "mcpm_plan_probe_particle_pitch": (C.c_int, [_plan, _f32p, C.c_int64, C.POINTER(C.c_int64)]),
    "mcpm_plan_set_particle_pitch": (C.c_int, [_plan, C.c_int64]),
    "mcpm_plan_particle_pitch": (C.c_int, [_plan, C.POINTER(C.c_int64)]),
    "mcpm_nbody_bf_vjp_f32": (C.c_int, [_plan, _f32p, C.c_int, _f64p, _f64p, C.c_double, _f64p, C.c_int, C.c_int, _f32p, _f32p, _f32p, _f32p, _f64p]),
    "mcpm_nbody_lightcone_f32": (C.c_int, [_plan, _f32p, C.c_int, C.c_double, C.c_double, _f32p, _f32p, _f32p, _f32p, _f32p]),
    "mcpm_nbody_bf_lc_vjp_f32": (C.c_int, [_plan, _f32p, C.c_int, _f64p, _f64p, C.c_double, C.c_double, _f64p, C.c_int, C.c_int, _f32p, _f32p,
                                           _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f64p]),
    "mcpm_slab_rccl_unique_id": (C.c_int, [C.c_void_p]),
    "mcpm_slab_comm_init_local": (C.c_int, [_plan]),
    "mcpm_slab_comm_init_rccl": (C.c_int, [_plan, C.c_void_p]),
    "mcpm_slab_comm_init_ops": (C.c_int, [_plan, C.c_void_p]),
    "mcpm_slab_comm_selftest": (C.c_int, [_plan]),
    "mcpm_slab_comm_shutdown": (C.c_int, [_plan]),
    "mcpm_slab_bind_workspace": (C.c_int, [_plan] + [_f32p] * 8),
    "mcpm_slab_step_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, _f32p, _f32p, _f32p]),
    "mcpm_slab_step_vjp_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, _f32p, _f32p,
                                        _d64p, _d64p, C.c_double, _d64p, C.c_int, C.c_double, C.c_double]),
    "mcpm_slab_dmax_seq": (C.c_int64, [_plan]),
    "mcpm_slab_dmax_read": (C.c_int, [_plan, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "mcpm_selftest_store3_nt": (C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int]),
    "mcpm_axpby_f32": (C.c_int, [_plan, _f32p, _f32p, C.c_int64, C.c_float, C.c_float, _f32p]),
    "mcpm_spectrum_workspace": (C.c_int, [C.c_int] * 7 + [C.POINTER(C.c_int64)]),
    "mcpm_spectrum_bins_c64": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _f32p, C.c_int64, _f32p, C.c_int64, C.c_int, _f64p, _f64p,
                                         _f64p, _f64p, C.c_int, _f64p, C.POINTER(C.c_int), C.c_int, _u8p, C.c_int64, _d64p]),
    "mcpm_binned_workspace": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "mcpm_binned_sums_f32": (C.c_int, [C.c_void_p, C.c_int64, _realp, C.c_int, _f32p, C.c_int64, _f32p, C.c_int64, C.c_double, _u8p, C.c_int,
                                       _f64p, C.c_int, _u8p, C.c_int64, _d64p]),
    "mcpm_bispectrum_workspace": (C.c_int, [C.c_int] * 6 + [C.POINTER(C.c_int64)]),
    "mcpm_bispectrum_split_c64": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _f32p, C.c_int64, C.c_int, _f64p, _f64p, _f64p, C.c_int,
                                            _f32p]),
    "mcpm_bispectrum_sums_f32": (C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int, C.c_int, _u32p, C.c_int, _u8p, C.c_int64, _d64p]),
    "mcpm_sky2cart_minmax_f64": (C.c_int, [_plan, _d64p, _d64p, _d64p, C.c_int64, _d64p, _d64p, C.c_int, _d64p, _d64p, _d64p]),
    "mcpm_sky2cell_f32": (C.c_int, [_plan, _d64p, _d64p, _d64p, C.c_int64, _d64p, _d64p, C.c_int, _f64p, _f64p, _f32p, _f32p]),
    "mcpm_box2cell_f32": (C.c_int, [_plan, _realp, _realp, C.c_int, C.c_int64, _f64p, _f64p, C.c_double, _f32p]),
    "mcpm_footprint_u8": (C.c_int, [_plan, _f32p, C.c_int64, _f32p, C.c_int, _u8p, C.c_int]),
    "mcpm_masked_sum_f64": (C.c_int, [_plan, _f32p, _u8p, C.c_int64, _d64p]),
    "mcpm_mclmc_kick_drift_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, _f32p, C.c_int64, C.c_double, C.c_double, _d64p]),
    "mcpm_mclmc_moments_f64": (C.c_int, [_plan, _f32p, C.c_int64, C.c_double, C.c_double, _d64p, _d64p]),
    "mcpm_chain_moments_f32": (C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                                         _d64p, _d64p]),
    "mcpm_chain_tau_f32": (C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                                     _d64p, _d64p, C.c_int, _d64p, _u32p]),
    "mcpm_bdec_sort_f32": (C.c_int, [C.c_void_p, _f32p, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int), C.c_int,
                                     _f32p, C.c_int64, _f32p, _u32p, _f32p, _u32p, _u32p, _f32p]),
    "mcpm_adam_step_f32": (C.c_int, [_plan, _f32p, _f32p, _f32p, _f32p, C.c_int64] + [C.c_double] * 6),
    "mcpm_probe_shift_f32": (C.c_int, [_plan, _f32p, C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_uint64, C.c_double, _f32p, _f32p]),
    "mcpm_hutchinson_accum_f64": (C.c_int, [_plan, _f32p, _f32p, C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_uint64, C.c_double, _d64p]),
    "mcpm_schur_f64": (C.c_int, [_plan, _f32p, C.c_int, C.c_int64, C.c_int64, _d64p, C.c_double, _d64p]),
    "mcpm_growth_table": (C.c_int, [C.c_double] * 6 + [C.c_int] + [_f64p] * 7),
    "mcpm_distance_table": (C.c_int, [C.c_double] * 6 + [C.c_int] + [_f64p] * 2),
}


ABI_VERSION = "mcpm 0.12 (gfx950)"   # must equal mcpm_version() of the loaded library (include/mcpm.h MCPM_ABI_VERSION)


def _load():
    build_log = ""
    if not os.path.exists(LIB_PATH) and os.path.exists("/opt/rocm/bin/hipcc"):
        # a fresh checkout (the .so is git-ignored): build the HIP library in-tree once; there is still no fallback
        import subprocess
        r = subprocess.run(["make", "-j8", "-C", os.path.join(_HERE, "csrc")], check=False, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            build_log = "\n--- tail of the failed `make -C montecosmo_amd/csrc` ---\n" + "\n".join(r.stdout.splitlines()[-30:])
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension is the product and there is no CPU fallback. "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C montecosmo_amd/csrc`." + build_log)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype, fn.argtypes = res, [C.c_void_p if issubclass(a, C.c_void_p) else a for a in args]
    got = lib.mcpm_version().decode()
    if got != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} reports ABI '{got}' but this package was written against '{ABI_VERSION}': "
                          "stale library, rebuild it with `make -C montecosmo_amd/csrc`.")
    return lib


lib = _load()


class McpmError(RuntimeError):
    pass


def check(rc, plan=None, what=""):
    if rc != OK:
        msg = lib.mcpm_last_error(plan)
        raise McpmError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")


# ------------------------------------------------------------------------------------------------
# the one call path: every argument that is a tensor or an array is checked against the table before the library is entered
# name -> per argument: the torch dtypes a device pointer accepts, HOST_F64, or () for anything that is not array data
KINDS = {name: tuple(_DEVICE_DTYPES.get(a, HOST_F64 if a is _f64p else ()) for a in args) for name, (_, args) in SIGNATURES.items()}
VALUE, CODE, PLAN_CODE = 0, 1, 2      # what a function returns: a value; a code for `check`; a code of the plan in argument 0
# name -> (function, number of arguments, positions that take array data, VALUE / CODE / PLAN_CODE)
_CALLS = {name: (getattr(lib, name), len(args), tuple(i for i, k in enumerate(KINDS[name]) if k),
                 VALUE if res is not C.c_int else PLAN_CODE if args[:1] == [_plan] else CODE)
          for name, (res, args) in SIGNATURES.items()}


def _tensor(name, i, t, kind, device):
    if kind is HOST_F64 or t.dtype not in kind:
        raise TypeError(f"{name}: argument {i} is a {t.dtype} tensor, expected {kind or 'no array'}")
    if (not t.is_cuda) if device is None else (t.device != device):
        raise ValueError(f"{name}: argument {i} is on {t.device}, expected {'a CUDA device' if device is None else device}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: argument {i} is not contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
    return t.data_ptr()


def _array(name, i, a, kind, device):
    if kind is not HOST_F64:
        raise TypeError(f"{name}: argument {i} is a numpy array, expected {'a device tensor' if kind else 'no array'}")
    if a.dtype != np.float64:
        raise TypeError(f"{name}: argument {i} is a {a.dtype} array, expected float64")
    if not a.flags.c_contiguous:
        raise ValueError(f"{name}: argument {i} is not C-contiguous (shape {a.shape}, strides {a.strides})")
    return a.ctypes.data_as(_f64p)


_CONVERT = {torch.Tensor: _tensor, torch.nn.Parameter: _tensor, np.ndarray: _array}


def marshal(name, args, device=None):
    """The C arguments of `name` for `args`: a tensor is checked (dtype of the pointer's kind, CUDA, on `device` if given, contiguous) and
    becomes its data pointer, a float64 C-contiguous numpy array a host double *; None, numbers and ctypes objects pass (positions from 0)."""
    if len(args) != _CALLS[name][1]:
        raise TypeError(f"{name} takes {_CALLS[name][1]} arguments, {len(args)} given")
    args = list(args)
    for i, a in enumerate(args):
        conv = _CONVERT.get(type(a))
        if conv is not None:
            args[i] = conv(name, i, a, KINDS[name][i], device)
    return args


def call(name, *args, device=None):
    """lib.<name>(*marshal(name, args, device)); a return code goes through `check`, any other result is returned."""
    fn, n, ptrs, result = _CALLS[name]
    if len(args) != n:
        raise TypeError(f"{name} takes {n} arguments, {len(args)} given")
    for i in ptrs:
        if type(args[i]) in _CONVERT:      # (when every pointer comes wrapped already, there is nothing to build)
            args = marshal(name, args, device)
            break
    try:
        r = fn(*args)
    except C.ArgumentError as e:      # a wrong type where a number belongs, refused before the library is entered; ctypes counts from 1
        marshal(name, args, device)      # (an array there gets the message of every other misplaced array)
        pos, what = re.match(r"argument (\d+): (.*)", str(e), re.S).groups()
        raise TypeError(f"{name}: argument {int(pos) - 1} {what}") from None
    if result == VALUE:
        return r
    if r != OK:
        check(r, args[0] if result == PLAN_CODE else None, name)


class Ctx(types.SimpleNamespace):
    """What a forward call keeps for its `*_vjp` twin: a plain bag of named values (compared and hashed by identity)."""
    __eq__, __ne__, __hash__ = object.__eq__, object.__ne__, object.__hash__
