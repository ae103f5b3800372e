"""CPU-only half of the bf16x3 weight-gradient mode (csrc/wgrad_x3_kernels.hip, swnerf/wgrad.py set_precision): the C ABI declares,
exports and binds swnerf_gemm_tn_group_x3 and it refuses a bad item before any launch; the precision switch and the creators' option;
and the yardstick itself - the float64 emulation of the three-term product (tests/wgrad_x3_ref.py) must sit inside the gate and the
1/16 condition that tests/test_gpu_wgrad_x3.py holds the kernel to, on the very operands of those tests."""
import re
from types import SimpleNamespace

import pytest
import torch

import wgrad_x3_ref as XR
from swnerf import _lib, runner, wgrad

# one valid item (include/swnerf.h swnerf_gemm_item, in field order; the pointers are never dereferenced: rejected first)
_ITEM = dict(A=16, lda=256, B=16, ldb=256, C=16, ldc=256, bias=None, B2=None, ldb2=0, Ni2=0, C2=None, ldc2=0,
             A2=None, lda2=0, No2=0, C3=None, ldc3=0, bias3=None)


def options(tmp, **over):
    """what the creators read (tests/test_runner_host.py)"""
    a = dict(expname="e", basedir=str(tmp), netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, lrate=5e-4, netchunk=1024 * 64,
             no_reload=True, ft_path=None, N_samples=64, N_importance=128, perturb=1., use_viewdirs=True, i_embed=0, multires=10,
             multires_views=4, raw_noise_std=1., dataset_type="blender", white_bkgd=True, no_ndc=False, lindisp=False,
             nerf_type="direct_temporal", not_zero_canonical=False, use_two_models_for_fine=True, do_half_precision=False, layer_num=2)
    a.update(over)
    return SimpleNamespace(**a)


@pytest.fixture(autouse=True)
def _restore_precision():
    prev = wgrad.PRECISION
    yield
    wgrad.set_precision(prev)


def test_header_declares_and_binding_exposes_the_entry():
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"int swnerf_gemm_tn_group_x3\(const swnerf_gemm_item\* items /\*HOST\*/, int n_items, int64_t M, void\* stream\);", text)
    assert "swnerf_gemm_tn_group_x3" in _lib.EXPORTS
    assert _lib.SIGNATURES["swnerf_gemm_tn_group_x3"] == _lib.SIGNATURES["swnerf_gemm_tn_group"]
    fn = _lib.lib().swnerf_gemm_tn_group_x3
    assert fn.argtypes[0] is _lib.ctype_of("const swnerf_gemm_item*")


def test_entry_rejects_bad_items_before_any_launch():
    """No GPU here: an item that got as far as a launch would fail with a HIP error code, not SWNERF_E_ARG."""
    L = _lib.lib()
    M = 8192
    group = lambda qs, n=None, m=M: L.swnerf_gemm_tn_group_x3((_lib.GemmItem * len(qs))(*[_lib.GemmItem(*q.values()) for q in qs]),
                                                             len(qs) if n is None else n, m, None)
    for change, text in ((dict(lda=255), b"bad main operands (lda=255 "),
                         (dict(B2=16, ldb2=96, Ni2=65, C2=16, ldc2=96), b"bad B2 rider"),
                         (dict(A2=16, lda2=4, No2=1, ldc3=256), b"bad A2 rider")):
        bad = {**_ITEM, **change}
        assert group([bad]) == _lib.E_ARG and text in L.swnerf_last_error() and L.swnerf_last_error().startswith(b"gemm_tn_group_x3: item 0: ")
        assert group([_ITEM, _ITEM, bad]) == _lib.E_ARG and b"item 2: " in L.swnerf_last_error(), change      # checked before the good ones run
    assert L.swnerf_gemm_tn_group_x3(None, 1, M, None) == _lib.E_ARG
    assert group([_ITEM], n=-1) == _lib.E_ARG and group([_ITEM], m=-1) == _lib.E_ARG
    assert group([{**_ITEM, "A": None}], m=0) == 0 and L.swnerf_gemm_tn_group_x3(None, 0, M, None) == 0


def test_set_precision_names_and_default():
    assert wgrad.DEFAULT_PRECISION == "fp32" and wgrad.PRECISION == "fp32"      # (the suite runs without SWNERF_WGRAD_PRECISION)
    assert wgrad.set_precision("bf16x3") == "fp32" and wgrad.PRECISION == "bf16x3"
    assert wgrad.set_precision("fp32") == "bf16x3" and wgrad.PRECISION == "fp32"
    for name in ("bf16", "fp16", "bf16x3-fine", "", None):
        with pytest.raises(ValueError, match="unknown precision"):
            wgrad.set_precision(name)
    assert wgrad.PRECISION == "fp32"


@pytest.mark.parametrize("create", ["create_nerf", "create_dnerf", "create_tnerf", "create_multires"])
def test_creator_option_sets_the_mode(tmp_path, create):
    fn = getattr(runner, create)
    fn(options(tmp_path, wgrad_precision="bf16x3"), device="cpu")
    assert wgrad.PRECISION == "bf16x3"
    fn(options(tmp_path), device="cpu")                                          # absent: the default
    assert wgrad.PRECISION == "fp32"
    with pytest.raises(ValueError, match="unknown precision 'fp16'"):
        fn(options(tmp_path, wgrad_precision="fp16"), device="cpu")
    if create != "create_nerf":                                                  # (the static reference runner has no such option)
        with pytest.raises(NotImplementedError):                                 # this mode is not apex amp
            fn(options(tmp_path, wgrad_precision="bf16x3", do_half_precision=True), device="cpu")


def test_fit2d_creator_option(tmp_path):
    runner.create_fit2d(SimpleNamespace(L=4, layer_num=2, wgrad_precision="bf16x3"), device="cpu")
    assert wgrad.PRECISION == "bf16x3"


@pytest.mark.parametrize("M,zeros", XR.CASES, ids=lambda v: str(v))
def test_emulation_is_inside_its_own_gate(M, zeros):
    """The three-term float64 product on the GPU tests' operands: inside the gate and the 1/16 condition, with room (the kernel
    adds fp32 accumulation on top).  And the condition discriminates: each two-term product fails it."""
    A, B = (T_[:, :256] for T_ in XR.operands(M, zeros))
    C0 = torch.randn((256, 256), generator=torch.Generator().manual_seed(M))
    _, three, no_lh, no_hl = XR.products(A, B)
    reference = XR.reference(A, B)
    r_gate, r_drop = XR.check(f"emulation M={M} zeros={zeros}", C0.double() + three, M, reference, C0)
    assert r_gate <= 0.01 and r_drop <= 1.0 / 160
    for two in (no_lh, no_hl):
        with pytest.raises(AssertionError, match="1/16"):
            XR.check("one cross term missing", C0.double() + two, M, reference, C0)
