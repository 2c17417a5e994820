"""The 7x7 / 2 RGB stem entries of the C ABI without a GPU: the header declares them, the library exports them, the ctypes binding
covers them, the host-only support query answers what the kernels implement, the existing ABI answers are unchanged, and the K-index
map of csrc/conv_stem_map.h -- compiled with g++ (tests/emul/stem_map_emul.cpp) -- reproduces the convolution and its weight
gradient in fp64 when numpy replays both GEMMs through it."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["cd_conv2d_stem_supported", "cd_conv2d_stem_fwd", "cd_conv2d_stem_wgrad", "cd_conv2d_stem_wgrad_workspace_floats"]


def _lib():
    from consistent_depth_amd import _native
    return _native.lib()


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_declared_exported_and_bound(name):
    from consistent_depth_amd import _native
    header = open(os.path.join(ROOT, "include", "consistent_depth_amd.h")).read()
    m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\);" % name, header)
    assert m, f"{name} is not declared in the header"
    assert name in _native.SIGNATURES
    assert hasattr(_lib(), name)
    # the binding has one ctypes argument per parameter of the declaration
    assert len(_native.SIGNATURES[name][1]) == len([p for p in m.group(1).split(",") if p.strip()])


@pytest.mark.parametrize("pass_", [0, 2])
def test_support_query(pass_):
    q = _lib().cd_conv2d_stem_supported
    for cin in (1, 3, 4):
        for cout in (8, 24, 64):
            assert q(pass_, 7, 2, cin, cout) == 1
            assert q(1, 7, 2, cin, cout) == 0                                     # no input gradient
            assert q(pass_, 7, 1, cin, cout) == 0 and q(pass_, 7, 3, cin, cout) == 0   # stride 1 and 3
            for ks in (3, 5, 11):
                assert q(pass_, ks, 2, cin, cout) == 0
    assert q(pass_, 7, 2, 0, 64) == 0 and q(pass_, 7, 2, 5, 64) == 0 and q(pass_, 7, 2, 8, 64) == 0
    assert q(pass_, 7, 2, 3, 7) == 0 and q(pass_, 7, 2, 3, 0) == 0


def test_support_query_rejects_unknown_passes():
    q = _lib().cd_conv2d_stem_supported
    assert q(-1, 7, 2, 3, 64) == 0 and q(3, 7, 2, 3, 64) == 0


def test_the_existing_abi_answers_are_unchanged():
    from consistent_depth_amd import _native
    assert _lib().cd_abi_version() == 11 == _native.ABI_VERSION
    for p in (0, 1, 2):
        assert _lib().cd_conv2d_strided_supported(p, 7, 2, 3, 64) == 0


def test_workspace_query_is_pure_host_and_refuses_other_geometries():
    f = _lib().cd_conv2d_stem_wgrad_workspace_floats
    assert f(64, 3, 7) >= 64 * 147 and f(8, 1, 7) >= 8 * 49 and f(40, 4, 7) >= 40 * 196
    assert f(64, 3, 3) == 0 and f(64, 8, 7) == 0 and f(4, 3, 7) == 0


def test_the_switch_is_read_from_the_environment(monkeypatch):
    from consistent_depth_amd.ops import conv as C
    monkeypatch.delenv("CD_AMD_CONV_STEM", raising=False)
    assert C.stem_enabled()
    monkeypatch.setenv("CD_AMD_CONV_STEM", "0")
    assert not C.stem_enabled()


def test_a_stem_layer_needs_no_packed_filter(monkeypatch):
    """A PackPool skips the stem layer (the kernels read the plain filter) unless a switch routes it back to the stride-1 path."""
    from consistent_depth_amd.ops.conv_layer import HipConv2d
    monkeypatch.delenv("CD_AMD_CONV_STEM", raising=False)
    monkeypatch.delenv("CD_AMD_CONV_STRIDED", raising=False)
    stem, other = HipConv2d(3, 64, 7, 2, 3, bias=False), HipConv2d(64, 64, 3, 2, 1, bias=False)
    if _lib().cd_get_conv_arith() >= 1:
        assert not stem._uses_packed()
    assert other._uses_packed() and HipConv2d(3, 64, 7, 1, 3)._uses_packed() and HipConv2d(8, 64, 7, 2, 3)._uses_packed()
    monkeypatch.setenv("CD_AMD_CONV_STEM", "0")
    assert stem._uses_packed()


@pytest.fixture(scope="module")
def stem_map(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stem") / "stem_map_emul"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "consistent_depth_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "emul", "stem_map_emul.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    consts = [int(v) for v in out[0].split()[1:]]
    maps = {(ln.split()[0], int(ln.split()[1])): np.array([int(v) for v in ln.split()[3:]]) for ln in out if ln.startswith(("FWD", "WGRAD"))}
    tile = np.array([int(ln.split()[2]) for ln in out if ln.startswith("TILE")])
    return consts, maps, tile


def _stage(x, rows, gy0, gx0, tile_word, RS):
    """The tile the kernels stage: `rows` x 72 input pixels from (gy0, gx0), zeros outside, columns de-interleaved by `tile_word`."""
    C, H, W = x.shape
    t = np.zeros(C * rows * RS)
    for ci in range(C):
        for r in range(rows):
            gy = gy0 + r
            if not 0 <= gy < H:
                continue
            for c in range(72):
                if 0 <= gx0 + c < W:
                    t[(ci * rows + r) * RS + tile_word[c]] = x[ci, gy, gx0 + c]
    return t


@pytest.mark.parametrize("cin", [1, 3, 4])
@pytest.mark.parametrize("hw", [(13, 7), (1, 5), (2, 2), (16, 64), (9, 65)], ids=lambda s: "x".join(map(str, s)))
def test_the_k_index_map_reproduces_the_convolution_and_its_weight_gradient(stem_map, cin, hw):
    import torch
    import torch.nn.functional as F
    (PW, RS, SF_TY, SF_ROWS, SW_TY, SW_ROWS), maps, tile_word = stem_map
    assert RS == 2 * PW and sorted(tile_word) == sorted(set(tile_word)) and tile_word.max() < RS
    H, W = hw
    Ho, Wo, cout = (H + 1) // 2, (W + 1) // 2, 5
    rng = np.random.default_rng(cin * 100 + H * 7 + W)
    x, w, dy = rng.standard_normal((cin, H, W)), rng.standard_normal((cout, cin, 7, 7)), rng.standard_normal((cout, Ho, Wo))
    wt = torch.tensor(w, requires_grad=True)
    y_ref = F.conv2d(torch.tensor(x)[None], wt, None, 2, 3)
    y_ref.backward(torch.tensor(dy)[None])
    K = cin * 49

    def replay(TY, ROWS, offs):
        """(y, dw) of one pass's tiling: A = the tile gathered through the map, padding columns zero."""
        assert len(offs) % 16 == 0 and (offs[:K] >= 0).all() and (offs[K:] == -1).all()
        wp = np.zeros((cout, len(offs)))
        wp[:, :K] = w.reshape(cout, K)
        y, dwp = np.zeros((cout, Ho, Wo)), np.zeros((cout, len(offs)))
        for Y0 in range(0, Ho, TY):
            for X0 in range(0, Wo, 32):
                t = _stage(x, ROWS, 2 * Y0 - 3, 2 * X0 - 4, tile_word, RS)
                for yy in range(min(TY, Ho - Y0)):
                    for i in range(min(32, Wo - X0)):
                        words = offs + 2 * yy * RS + i
                        assert words[:K].max() < len(t)
                        a = np.where(offs >= 0, t[np.maximum(words, 0)], 0.0)
                        y[:, Y0 + yy, X0 + i] = wp @ a
                        dwp += np.outer(dy[:, Y0 + yy, X0 + i], a)
        return y, dwp[:, :K].reshape(w.shape)

    y_f, _ = replay(SF_TY, SF_ROWS, maps[("FWD", cin)])
    _, dw_w = replay(SW_TY, SW_ROWS, maps[("WGRAD", cin)])
    assert len(maps[("WGRAD", cin)]) % 32 == 0
    assert np.abs(y_f - y_ref[0].detach().numpy()).max() <= 1e-12
    assert np.abs(dw_w - wt.grad.numpy()).max() <= 1e-12
