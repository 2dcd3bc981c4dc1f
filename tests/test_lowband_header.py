"""The low-band inverse transforms of the coarse decoders (dctz_amd/csrc/dct_lowband_block.h: the code one GPU lane
executes) compiled for the CPU (tests/emu/emu_lowband.cpp) against the definition in float64,
    y[i] = sum_{k < K} alpha_N(k) c[k] cos(pi k (2i + 1) / (2K)).
y is the K-point ORTHONORMAL DCT-III of sqrt(K/N) c[0 .. K-1], so the yardstick of tests/noise.py applies to a block of
that norm: |y - reference| <= K_NOISE eps(T) sqrt(K/N) ||c[0 .. K-1]||_2 (per axis for the tiles)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.noise import K_NOISE

HERE = os.path.dirname(os.path.abspath(__file__))


def basis(N, K):
    """B[i, k] = alpha_N(k) cos(pi k (2i + 1) / (2K)), k < K.  The angle is reduced in integers first (k (2i + 1) mod 4K):
    at k (2i + 1) ~ 2000 the rounding of the product with pi alone would cost the cosine 30 eps."""
    i = np.arange(K)[:, None]
    k = np.arange(K)[None, :]
    alpha = np.where(k == 0, np.sqrt(1.0 / N), np.sqrt(2.0 / N))
    return alpha * np.cos(np.pi * ((k * (2 * i + 1)) % (4 * K)) / (2 * K))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "emu_lowband.so")
    src = os.path.join(HERE, "emu", "emu_lowband.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-mfma", "-shared", "-fPIC", "-o", so, src])
    lib = C.CDLL(so)
    lib.emu_lowband_cos.restype = C.c_double
    return lib


def _vectors(rng, count, size, dtype):
    for i in range(count):
        c = (rng.standard_normal(size) * 10 ** rng.uniform(-3, 3)).astype(dtype)
        if i == 0:
            c[:] = 0
        if i == 1:
            c[:] = 0
            c[0] = 8.0
        if i == 2:
            c[:] = 1
        yield c


def test_cosine_table(emu):
    for m in range(0, 400):
        # (the reference's argument is below 2 pi: its rounding moves the cosine by less than 1e-15)
        assert abs(emu.emu_lowband_cos(m) - np.cos(np.pi * (m % 128) / 64)) <= 1e-15


@pytest.mark.parametrize("dtype,suf", [(np.float64, "f64"), (np.float32, "f32")])
@pytest.mark.parametrize("N,K", [(64, 1), (64, 2), (64, 4), (64, 8), (64, 16), (64, 32), (8, 1), (8, 2), (8, 4), (4, 1), (4, 2)])
def test_one_dimension(emu, dtype, suf, N, K):
    B = basis(N, K)
    eps = float(np.finfo(dtype).eps)
    fn = getattr(emu, "emu_lowband_" + suf)
    rng = np.random.default_rng(100 * N + K)
    for c in _vectors(rng, 300, K, dtype):
        y = np.empty(K, dtype)
        assert fn(N, K, c.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)) == 0
        want = B @ c.astype(np.float64)
        tol = K_NOISE * eps * np.sqrt(K / N) * np.linalg.norm(c.astype(np.float64))
        assert np.all(np.abs(y.astype(np.float64) - want) <= tol + 1e-300), (N, K, np.abs(y - want).max(), tol)
        # the mean of the K values is the block mean of the full reconstruction: c[0] / sqrt(N)
        assert abs(y.astype(np.float64).mean() - float(c[0]) / np.sqrt(N)) <= tol + 1e-300
    assert fn(N, 3, None, None) == -1


@pytest.mark.parametrize("dtype,suf", [(np.float64, "f64"), (np.float32, "f32")])
@pytest.mark.parametrize("geom,K", [(1, 2), (1, 4), (2, 2)])
def test_tiles_are_separable(emu, dtype, suf, geom, K):
    N, nd = (8, 2) if geom == 1 else (4, 3)
    B = basis(N, K)
    eps = float(np.finfo(dtype).eps)
    fn = getattr(emu, "emu_lowband_tile_" + suf)
    rng = np.random.default_rng(10 * geom + K)
    for c in _vectors(rng, 300, K ** nd, dtype):
        v = c.copy()
        assert fn(geom, K, v.ctypes.data_as(C.c_void_p)) == 0
        a = c.astype(np.float64).reshape((K,) * nd)
        want = np.einsum("ik,jl,kl->ij", B, B, a) if nd == 2 else np.einsum("ia,jb,kc,abc->ijk", B, B, B, a)
        tol = nd * K_NOISE * eps * np.sqrt(K / N) ** nd * np.linalg.norm(a)
        assert np.all(np.abs(v.astype(np.float64) - want.ravel()) <= tol + 1e-300), (geom, K)
