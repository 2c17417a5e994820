"""The stride-2 convolution entries of the C ABI without a GPU: the header declares them, the library exports them, the ctypes
binding covers them, and the host-only support query answers what the kernels implement."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["cd_conv2d_strided_supported", "cd_conv2d_fwd_strided", "cd_conv2d_dgrad_strided", "cd_conv2d_wgrad_strided",
           "cd_subsample2_fwd", "cd_subsample2_bwd"]


def _lib():
    from consistent_depth_amd import _native
    return _native.lib()


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_declared_exported_and_bound(name):
    from consistent_depth_amd import _native
    header = open(os.path.join(ROOT, "include", "consistent_depth_amd.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in the header"
    assert name in _native.SIGNATURES
    assert hasattr(_lib(), name)
    # the binding has one ctypes argument per parameter of the declaration
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1)
    assert len(_native.SIGNATURES[name][1]) == len([p for p in decl.split(",") if p.strip()])


def test_abi_version_is_11():
    from consistent_depth_amd import _native
    assert _lib().cd_abi_version() == 11 == _native.ABI_VERSION
    assert re.search(r"#define\s+CD_ABI_VERSION\s+11\b", open(os.path.join(ROOT, "include", "consistent_depth_amd.h")).read())


@pytest.mark.parametrize("pass_", [0, 1, 2])
def test_support_query(pass_):
    q = _lib().cd_conv2d_strided_supported
    for c in (8, 16, 64, 128):
        assert q(pass_, 3, 2, c, c) == 1
        assert q(pass_, 1, 2, c, c) == 1
        assert q(pass_, 3, 1, c, c) == 0 and q(pass_, 3, 3, c, c) == 0      # stride 1 and 3
        assert q(pass_, 5, 2, c, c) == 0 and q(pass_, 11, 2, c, c) == 0    # no model strides these filters
    assert q(pass_, 3, 2, 16, 40) == 1 and q(pass_, 3, 2, 40, 8) == 1
    # the RGB stems (7x7 / 2 on 3 channels) are not built: fewer than 8 input channels keep the stride-1-plus-sub-sampling path
    assert q(pass_, 7, 2, 3, 64) == 0 and q(pass_, 3, 2, 3, 64) == 0 and q(pass_, 3, 2, 7, 64) == 0
    assert q(pass_, 3, 2, 0, 8) == 0 and q(pass_, 3, 2, 8, 0) == 0


def test_support_query_rejects_unknown_passes():
    q = _lib().cd_conv2d_strided_supported
    assert q(-1, 3, 2, 16, 16) == 0 and q(3, 3, 2, 16, 16) == 0


def test_the_switch_is_read_from_the_environment(monkeypatch):
    from consistent_depth_amd.ops import conv as C
    monkeypatch.delenv("CD_AMD_CONV_STRIDED", raising=False)
    assert C.strided_enabled()
    monkeypatch.setenv("CD_AMD_CONV_STRIDED", "0")
    assert not C.strided_enabled()
