"""`png_type` in model-argument files (montecosmo_amd/register.py): 'fNL' / 'bias' reach FieldLevelForward's arguments, the string
'None' (how an HDF5 / npz file carries a None) and an absent key both mean no primordial non-Gaussianity; the key survives a file."""
import numpy as np
import pytest


def _reg(png_type="absent"):
    rng = np.random.default_rng(5)
    reg = dict(cell_length=25., box_center=np.array([10., -20., 1500.]), box_rotvec=np.array([0.1, 0., -0.2]), init_oversamp=1.5,
               paint_oversamp=1.75, cosmo_fid=dict(Omega_m=0.3137721, sigma8=0.8076354), count_mesh=rng.poisson(3.0, (8, 6, 10)).astype(np.float64),
               a_obs=0.6, curved_sky=False)
    if png_type != "absent":
        reg["png_type"] = png_type
    return reg


@pytest.mark.parametrize("png_type,want", [("fNL", "fNL"), ("bias", "bias"), ("None", None), (None, None), ("absent", None)])
def test_model_arguments_png_type(png_type, want):
    from montecosmo_amd import register
    fwd = register.model_arguments(_reg(png_type))["forward"]
    assert fwd.get("png_type") == want


def test_png_type_round_trip(tmp_path):
    from montecosmo_amd import register
    path = register.save_register(str(tmp_path / "reg.npz"), _reg("fNL"))
    assert register.model_arguments(register.load_register(path))["forward"]["png_type"] == "fNL"
