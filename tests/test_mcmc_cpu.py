"""CPU: MCMC densification without a device.  The float64 reference (tests/mcmc_ref.py) against the properties of the
published split rule; the C entries' argument checks, which sit in front of their first HIP call; the strategy's growth
arithmetic and its refusal of host tensors."""
import ctypes
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import mcmc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", [0.005, 0.3, 0.99, 1 - 6e-8])
def test_one_copy_is_the_identity(o):
    o_new, ratio = R.split(o, 1)
    assert abs(o_new - o) <= 1e-15 * o and abs(ratio - 1.0) <= 1e-12


@pytest.mark.parametrize("o", [0.005, 0.3, 0.99, 1 - 6e-8])
@pytest.mark.parametrize("N", [2, 3, 17, 51])
def test_n_copies_leave_the_transmittance_unchanged(o, N):
    o_new, _ = R.split(o, N)
    assert abs((1.0 - o_new) ** N - (1.0 - o)) <= 1e-12


@pytest.mark.parametrize("o, N, want", [(0.005, 51, 0.999281), (0.3, 51, 0.951073), (0.99, 51, 0.642124), (1 - 6e-8, 51, 0.501459)])
def test_scale_ratio_values(o, N, want):
    """s'/s computed in extended precision for the issue; six decimals are given."""
    assert abs(R.split(o, N)[1] - want) <= 1e-6


@pytest.mark.parametrize("o", [0.005, 0.3, 0.99, 1 - 6e-8])
def test_scale_ratio_decreases_with_the_number_of_copies(o):
    ratios = [R.split(o, N)[1] for N in range(1, 52)]
    assert all(b < a for a, b in zip(ratios, ratios[1:]))


def test_noise_gate():
    """g(0.005) is 0.5 exactly; 0.37 leaves room for the float32 rounding of 1 - o at the steep point (slope 100)."""
    for T in (np.float64, np.float32):
        assert R.gate(np.array([0.005], dtype=T))[0] > 0.37
        assert R.gate(np.array([0.99], dtype=T))[0] < 1e-40
    assert abs(R.gate(np.array([0.005]))[0] - 0.5) < 1e-12


def test_float32_restatement_is_close_to_the_reference():
    """The calibration path computes the same thing: relocation on a few rows, float32 against float64."""
    rng = np.random.default_rng(0)
    P = 8
    params = {"xyz": rng.uniform(-1, 1, (P, 3)).astype(np.float32), "f_dc": rng.normal(size=(P, 1, 3)).astype(np.float32),
              "f_rest": rng.normal(size=(P, 2, 3)).astype(np.float32), "rotation": rng.normal(size=(P, 4)).astype(np.float32),
              "opacity": rng.uniform(-4, 4, (P, 1)).astype(np.float32), "scaling": rng.uniform(-6, -1, (P, 3)).astype(np.float32)}
    dst, src = [0, 1, 2], [4, 4, 5]
    a, _ = R.relocate(params, None, dst, src)
    b, _ = R.relocate(params, None, dst, src, dtype=np.float32)
    assert b["opacity"].dtype == np.float32 and a["opacity"].dtype == np.float64
    assert np.abs(a["opacity"] - b["opacity"]).max() < 1e-5 and np.abs(a["scaling"] - b["scaling"]).max() < 1e-5
    assert np.array_equal(a["xyz"][0], params["xyz"][4]) and np.array_equal(a["xyz"][3], params["xyz"][3])
    assert np.array_equal(a["opacity"][[3, 6, 7]], params["opacity"][[3, 6, 7]].astype(np.float64))


# ---- the C ABI on a machine without a device -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from luciddreamer_amd import _lib, build
    build.build()
    return _lib.lib()


def test_symbols_are_exported(L):
    for name in ("lr_mcmc_relocate", "lr_mcmc_workspace_bytes", "lr_mcmc_noise", "lr_mcmc_reg_grad"):
        assert hasattr(L, name), name
    from luciddreamer_amd import _lib
    assert set(n for n in _lib.EXPORTS if "mcmc" in n) == {"lr_mcmc_relocate", "lr_mcmc_workspace_bytes", "lr_mcmc_noise",
                                                             "lr_mcmc_reg_grad"}


def test_workspace_size_is_a_pure_host_function(L):
    w = L.lr_mcmc_workspace_bytes
    assert w(1, 0) > 0 and w(1000, 10) % 256 == 0
    assert w(1000, 10) < w(2000, 10) < w(1_000_000, 10)
    assert w(1000, 10) < w(1000, 1000) < w(1000, 100_000)
    assert w(1000, 10) >= 1000 * 4 + 10 * 16 + (51 * 51 + 51) * 8        # counts, staged results, the binomial table


def test_ctypes_structure_mirrors_the_header(tmp_path):
    from luciddreamer_amd import _lib
    S = _lib.McmcRelocateArgs
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no host C compiler"
    members = [(f[0], getattr(S, f[0]).offset, getattr(S, f[0]).size) for f in S._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lucid_raster.h"\nint main(void)\n{\n'
                   '    printf("sizeof %zu\\n", sizeof(lr_mcmc_relocate_args));\n' +
                   "".join(f'    printf("{n} %zu %zu\\n", offsetof(lr_mcmc_relocate_args, {n}), '
                           f'sizeof(((lr_mcmc_relocate_args*)0)->{n}));\n' for n, _, _ in members) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert lines[0] == f"sizeof {ctypes.sizeof(S)}"
    assert lines[1:1 + len(members)] == [f"{n} {o} {s}" for n, o, s in members]
    end = 0
    for n, o, s in members:                      # every member of the C struct is mirrored: no gap beyond alignment padding
        assert 0 <= o - end < 8, n
        end = o + s
    assert 0 <= ctypes.sizeof(S) - end < 8


_BUF = (ctypes.c_float * 72)()
PTR = (ctypes.addressof(_BUF) + 15) & ~15               # non-NULL, 16-byte aligned, never dereferenced by the checks


def _args(**fields):
    from luciddreamer_amd import _lib
    a = dict(n=4, dst=PTR, src=PTR, P_rows=100, M=16, xyz=PTR, features_dc=PTR, features_rest=PTR, opacity=PTR, scaling=PTR,
             rotation=PTR, min_opacity=0.005, n_max=51, workspace=PTR, workspace_bytes=1 << 20)
    a.update(fields)
    return _lib.McmcRelocateArgs(**a)


REJECTED = {
    "negative_n": (dict(n=-1), b"n must be"),
    "n_max_zero": (dict(n_max=0), b"n_max"),
    "n_max_52": (dict(n_max=52), b"n_max"),
    "no_rows": (dict(P_rows=0), b"P_rows"),
    "no_dst": (dict(dst=None), b"dst and src"),
    "no_src": (dict(src=None), b"dst and src"),
    "no_xyz": (dict(xyz=None), b"parameter tensors"),
    "no_features_dc": (dict(features_dc=None), b"parameter tensors"),
    "no_features_rest": (dict(features_rest=None), b"parameter tensors"),
    "no_opacity": (dict(opacity=None), b"parameter tensors"),
    "no_scaling": (dict(scaling=None), b"parameter tensors"),
    "no_rotation": (dict(rotation=None), b"parameter tensors"),
    "no_workspace": (dict(workspace=None), b"workspace"),
    "small_workspace": (dict(workspace_bytes=64), b"workspace"),
}


@pytest.mark.parametrize("case", sorted(REJECTED))
def test_relocate_rejects_without_a_device(L, case):
    from luciddreamer_amd import _lib
    fields, message = REJECTED[case]
    assert L.lr_mcmc_relocate(_args(**fields)) == _lib.LR_ERR_INVALID_ARG
    assert message in L.lr_last_error()


def test_relocate_checks_struct_bytes_first(L):
    from luciddreamer_amd import _lib
    assert L.lr_mcmc_relocate(None) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()
    a = _args()
    a.struct_bytes -= 8
    assert L.lr_mcmc_relocate(a) == _lib.LR_ERR_INVALID_ARG and b"struct_bytes" in L.lr_last_error()


def test_relocate_of_no_pairs_returns_zero(L):
    assert L.lr_mcmc_relocate(_args(n=0)) == 0                                    # no device is touched
    assert L.lr_mcmc_relocate(_args(n=0, dst=None, src=None, workspace=None, workspace_bytes=0)) == 0
    assert L.lr_mcmc_relocate(_args(n=0, M=1, features_rest=None)) == 0           # a degree-0 model has no features_rest


def test_noise_and_regulariser_reject_without_a_device(L):
    from luciddreamer_amd import _lib
    assert L.lr_mcmc_noise(0, None, None, None, None, None, 1.0, None) == 0
    assert L.lr_mcmc_noise(-1, PTR, PTR, PTR, PTR, PTR, 1.0, None) == _lib.LR_ERR_INVALID_ARG
    assert L.lr_mcmc_noise(10, PTR, PTR, PTR, PTR, None, 1.0, None) == _lib.LR_ERR_INVALID_ARG and b"noise" in L.lr_last_error()
    assert L.lr_mcmc_noise(10, PTR, PTR, PTR + 4, PTR, PTR, 1.0, None) == _lib.LR_ERR_INVALID_ARG and b"aligned" in L.lr_last_error()
    assert L.lr_mcmc_reg_grad(0, None, None, 0.01, 0.01, None, None, None) == 0
    assert L.lr_mcmc_reg_grad(10, PTR, PTR, 0.01, 0.01, None, PTR, None) == _lib.LR_ERR_INVALID_ARG
    assert b"gradient" in L.lr_last_error()


# ---- the strategy ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap_max, want", [(5000, 50), (1020, 20), (1000, 0), (900, 0)])
def test_growth_arithmetic(cap_max, want):
    from luciddreamer_amd.mcmc import MCMCStrategy
    assert MCMCStrategy(cap_max).n_new(1000) == want


def test_package_exports_the_module():
    import luciddreamer_amd
    assert luciddreamer_amd.mcmc.MCMCStrategy is not None


def _host_model(P=10):
    mk = lambda *s: torch.nn.Parameter(torch.rand(*s))
    m = types.SimpleNamespace(_xyz=mk(P, 3), _features_dc=mk(P, 1, 3), _features_rest=mk(P, 15, 3), _opacity=mk(P, 1),
                              _scaling=mk(P, 3), _rotation=mk(P, 4))
    names = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
             "rotation": "_rotation"}
    m.optimizer = torch.optim.Adam([{"params": [getattr(m, a)], "lr": 1e-3, "name": n} for n, a in names.items()], lr=0.0)
    return m


def test_host_tensors_raise():
    from luciddreamer_amd import mcmc
    s, m = mcmc.MCMCStrategy(100), _host_model()
    for call in (lambda: s.relocate(m), lambda: s.grow(m), lambda: s.inject_noise(m, 1.6e-4), lambda: s.add_regularizer_grads(m),
                 lambda: s.step(m, 500, 1.6e-4)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
    with pytest.raises(RuntimeError, match="HIP device"):
        mcmc.add_noise(m._xyz.detach(), m._scaling.detach(), m._rotation.detach(), m._opacity.detach(), torch.zeros(10, 3), 1.0)
