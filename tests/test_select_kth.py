"""CPU: the bit-sliced k-th-smallest-magnitude search of the compression kernel (mustafar_amd/csrc/select_kth.h, shared by the
device code and this host build) against numpy on random, tie-heavy and degenerate rows; k as the prune rule makes it
(models/llama_mustafar_kernel.py:88-103: k = max(1, int(s * 128)), kthvalue = k-th smallest magnitude)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("selkth") / "libselect_kth_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "csrc", "select_kth_host.cpp"), "-o", out])
    L = ctypes.CDLL(out)
    L.kth_rows.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.transpose_block.argtypes = [ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def devlib(tmp_path_factory):
    """The device branch of the header (byte permutes instead of shift + select) built for the host with a model of v_perm_b32."""
    out = str(tmp_path_factory.mktemp("selkth_dev") / "libselect_kth_device_emu.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "csrc", "select_kth_device_emu.cpp"), "-o", out])
    L = ctypes.CDLL(out)
    L.kth_rows.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return L


def test_transpose_orientation(lib):
    rng = np.random.default_rng(0)
    a = rng.integers(0, 2 ** 32, 32, dtype=np.uint64).astype(np.uint32)
    t = a.copy()
    lib.transpose_block(t.ctypes.data)
    for b in range(32):
        for i in range(32):
            assert (int(t[31 - b]) >> (31 - i)) & 1 == (int(a[i]) >> b) & 1


def _rows():
    rng = np.random.default_rng(1)
    rows = [rng.standard_normal((400, 128)).astype(np.float16)]
    rows.append((rng.integers(-3, 4, (200, 128)) * 0.5).astype(np.float16))            # heavy ties, zeros, both signs
    rows.append(np.zeros((3, 128), np.float16))
    rows.append(np.full((2, 128), -0.0, np.float16))
    rows.append((rng.standard_normal((50, 128)) * 1e-6).astype(np.float16))             # subnormals
    big = rng.standard_normal((50, 128)).astype(np.float32) * 3e4
    rows.append(np.clip(big, -65504, 65504).astype(np.float16))                         # up to the largest finite magnitude
    one = np.zeros((4, 128), np.float16); one[:, 77] = 5.0
    rows.append(one)
    return np.concatenate(rows)


@pytest.mark.parametrize("kth", [1, 2, 38, 64, 89, 102, 126, 127, 128])
def test_kth_magnitude_matches_numpy(lib, kth):
    x = _rows()
    mags = (x.view(np.uint16) & 0x7fff)
    want = np.sort(mags, axis=1)[:, kth - 1].astype(np.uint32)
    words = np.ascontiguousarray(x.view(np.uint16)).view(np.uint32).reshape(x.shape[0], 64)   # element 2j low, 2j + 1 high
    got = np.empty(x.shape[0], np.uint32)
    lib.kth_rows(words.ctypes.data, x.shape[0], kth, got.ctypes.data)
    assert np.array_equal(got, want)


def test_device_branch_kth_matches_numpy_at_every_k(devlib):
    """What the GPU build compiles (the perm stages, SERIAL both ways), at every k 1..128.  (Exchanging the selectors of the two
    permutes of one stage, or the operands of one permute, only relabels which element sits at which bit of every plane -- the
    search reads counts and intersections and gives the same result; a permute given a wrong selector does not.)"""
    x = _rows()
    mags = np.sort(x.view(np.uint16) & 0x7fff, axis=1)
    words = np.ascontiguousarray(x.view(np.uint16)).view(np.uint32).reshape(x.shape[0], 64)
    got = np.empty(x.shape[0], np.uint32)
    for kth in range(1, 129):
        for serial in (0, 1):
            devlib.kth_rows(words.ctypes.data, x.shape[0], kth, serial, got.ctypes.data)
            bad = np.nonzero(got != mags[:, kth - 1])[0]
            assert not len(bad), f"kth {kth} serial {serial}: rows {bad[:8].tolist()}"
