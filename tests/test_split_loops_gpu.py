"""The K loops of the exact split (csrc/split_core.h) with operands that carry all 24 significand bits, bit for bit.

The split is written as single instructions (vd_split3: conversion, unpack, subtraction) and the step kernel's half step is peeled out
of its main loop.  What can go wrong there is a plane lost or mis-assembled and the peeled tail; the one-hot cases of
tests/test_split_shape_gpu.py multiply small integers, whose mid and lo planes are zero, and would not notice.  Here one operand is
random full-mantissa fp32 (randn times a random power of two) and the other has ONE non-zero per output column, a signed power of two:
every output element is a single product v * 2^e, exact in fp32, and every other term of its sum is an exact zero, so neither the order
of the nine plane products nor the order of the split-K atomics matters.  A dropped lo plane shows as a relative error of about
2^-18 ~ 3.8e-6 in most elements, a dropped mid plane as 2^-9; both fail np.array_equal.

  * dWh contraction (gemm_split_tn_kernel<9>) through ops.gemm_tn_acc with FLAG_SPLIT9: both operands are split in registers, so each
    side takes the random operand once.  Shapes: the K threshold with one tile, and four tiles with a ragged last K range.
  * step kernel (gemm_split_kernel<9>) through vd_img_tr_backward_p with its attention term zeroed (p = datt = 0, dpre = 0: the
    epilogue adds acc + 0 * 0 onto 0).  The recurrence's own read-out of this product, dh0 of vd_lstm_backward, is computed by the fp32
    kernel, so the image product is the exact read-out.  K walks the tail only (16), one full step (32), full + half (48), two full
    (64: the main loop runs once), 80, 96 and 112 (the main loop runs twice: both LDS stages)."""
import numpy as np
import pytest
import torch

import attention_ref as ar
import test_ops_gpu as tog
from test_attention_ops_gpu import internal, ops, ptr, stream  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def full_mantissa(rng, *shape):
    """fp32 values with random low significand bits over 13 binades"""
    return (rng.randn(*shape) * np.exp2(rng.randint(-6, 7, size=shape))).astype(np.float32)


def one_hot_pow2(rng, K, n, emax, signed):
    """[K x n]: column j holds (+-) 2^e_j at row k_j and zeros elsewhere; the first and the last row of K are among the k_j"""
    k = rng.randint(0, K, size=n)
    k[0], k[-1] = K - 1, 0
    w = np.exp2(rng.randint(-emax, emax + 1, size=n)).astype(np.float32)
    if signed:
        w *= np.where(rng.rand(n) < 0.5, -1, 1).astype(np.float32)
    m = np.zeros((K, n), np.float32)
    m[k, np.arange(n)] = w
    return m, k, w


def first_difference(got, ref):
    bad = np.argwhere(got != ref)
    return '%d of %d elements differ, first %s: got %r want %r (relative %.3e)' % (
        len(bad), ref.size, tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])],
        abs(float(got[tuple(bad[0])]) - float(ref[tuple(bad[0])])) / max(abs(float(ref[tuple(bad[0])])), 1e-30))


# (M, N, K): the K threshold of the split contraction with one 256 x 128 tile | four tiles, K = 16 * 515: a ragged last K range
TN_SHAPES = [(256, 128, 8192), (512, 256, 8240)]


@pytest.mark.parametrize("side", ['A', 'B'])
@pytest.mark.parametrize("M,N,K", TN_SHAPES)
def test_dwh_contraction_exact(ops, M, N, K, side):
    """C = A^T B with C zeroed: side A -> A random, B one-hot: C[m, n] = A[k_n, m] * 2^e_n; side B -> the roles swapped"""
    rng = np.random.RandomState(M + 3 * N + 7 * K + (side == 'B'))
    if side == 'A':
        A = full_mantissa(rng, K, M)
        B, k, w = one_hot_pow2(rng, K, N, 8, False)
        ref = A[k, :].T * w[None, :]
    else:
        B = full_mantissa(rng, K, N)
        A, k, w = one_hot_pow2(rng, K, M, 8, False)
        ref = B[k, :] * w[:, None]
    out = ar.Guarded((M, N), init=np.zeros((M, N), np.float32))
    Ad, Bd = tog.dev(A), tog.dev(B)
    ops.gemm_tn_acc(Ad, Bd, out.t, flags=ops.FLAG_SPLIT9)
    torch.cuda.synchronize()
    got = out.t.cpu().numpy()
    assert np.array_equal(got, ref), 'dWh side %s (%d, %d, %d): %s' % (side, M, N, K, first_difference(got, ref))
    assert not out.written_guard_rows()


@pytest.mark.parametrize("K", [16, 32, 48, 64, 80, 96, 112])
@pytest.mark.parametrize("rows", [128, 129])
def test_step_kernel_exact(ops, internal, rows, K):
    """dpre = dz Wc: dz random full-mantissa (the operand the step kernel splits in registers), Wc one signed power of two per output
    column; H = 144 output columns (a ragged second column tile); rows = one workgroup, and one row into the second"""
    H = 144
    rng = np.random.RandomState(rows * 131 + K)
    dz = full_mantissa(rng, rows, K)
    Wc, k, w = one_hot_pow2(rng, K, H, 8, True)
    ref = dz[:, k] * w[None, :]
    out = ar.Guarded((rows, H), init=np.zeros((rows, H), np.float32))
    dzd, Wd = tog.dev(dz), tog.dev(Wc)
    pd, dd = torch.zeros(rows, device='cuda'), torch.zeros(rows, H, device='cuda')
    internal.tr_backward(ptr(dzd), ptr(Wd), ptr(pd), ptr(dd), None, ptr(out.t), rows, 1, 1, H, K, 1.0, ops.FLAG_SPLIT9, stream())
    torch.cuda.synchronize()
    got = out.t.cpu().numpy()
    assert np.array_equal(got, ref), 'step kernel rows %d K %d: %s' % (rows, K, first_difference(got, ref))
    assert not out.written_guard_rows()
