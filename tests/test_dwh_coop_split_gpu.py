"""The weight-gradient contraction of the exact split (csrc/split_core.h gemm_split_tn_kernel) with its B tile split once per workgroup.

Per 16-k step wave w splits column tile w of the shared [16 k][128 n] tile, stores the three planes over the fp32 quarter it has read, a
barrier publishes them and every wave reads all four tiles' planes.  What can go wrong there: a wave reads another wave's quarter or a
plane of the step before (a missing or misplaced barrier), the next stage's DMA lands on planes still being read, the odd tail step uses
the wrong stage, a plane is lost.  Every case below therefore uses a B (and an A) that differs in every element, full-mantissa fp32, so
that all three planes of every value carry bits, and the kernel is called alone through the internal entry point vd_gemm_split_tn_p
(bound by visdial_amd._lib.internal), below the K thresholds of vd_gemm_tn_acc.

Shapes (M, N, K), the smallest at which this kernel takes another path:
  (256, 128, 16) / 32 / 48   one workgroup: one step (stage 0), two (both stages), three (the odd tail step back on stage 0)
  (256, 128, 576)            64 * 9: nine K ranges of 64 rows rounded up to 16 workgroups -- seven leave at once, the XCD map is on
  (256, 128, 528)            a ragged last K range: eight of 64 rows and one of 16
  (512, 256, 2048)           four tiles per K range, 32 ranges over the XCDs
  (512, 256, 2096)           the same with a last range of 48 rows

Exact cases: one operand is random, the other has ONE non-zero per output row / column, a power of two, so every output element is a
single exact product and every other term an exact zero: the result is compared bit for bit with the fp64 product (neither the order of
the nine products nor of the split-K atomics matters).  With nprod = 1 (the bf16 pass: hi planes only) the random operand is rounded to
bf16 first, which makes the same statement exact there.  The one-hot rows walk every k of short K.

Random cases, rel-L2 against fp64.  The products of the planes are exact, so the error is that of adding them in fp32: 9 K additions per
element, each rounding by at most 2^-24 of a partial sum no larger (rms) than the result's scale, independent: sqrt(9 K) * 2^-24, times 4
for the MFMA's internal order and the atomics, capped by the suite's split9 bound of 2e-5 (tests/test_ops_gpu.py):
min(12 * sqrt(K) * 2^-24, 2e-5).  nprod = 1 is held to the same bound against the fp64 product of the bf16-ROUNDED operands (K additions,
fewer than 9 K): what it drops is the rounding of the operands and nothing else.

Two launches back to back into the same C must give exactly twice one launch's sum in the exact cases (C + C is exact), and the random
case is accumulated onto a non-zero C."""
import functools

import numpy as np
import pytest
import torch

import attention_ref as ar
import test_ops_gpu as tog
from test_attention_ops_gpu import acc_init, ops, ptr, stream  # noqa: F401  (fixtures)
from test_split_loops_gpu import first_difference, full_mantissa

pytestmark = pytest.mark.gpu

SHAPES = [(256, 128, 16), (256, 128, 32), (256, 128, 48), (256, 128, 576), (256, 128, 528), (512, 256, 2048), (512, 256, 2096)]


@pytest.fixture(scope="module")
def split_tn(ops):
    from visdial_amd import _lib
    return _lib.internal('vd_gemm_split_tn_p')


def to_bf16(a):
    """fp32 -> the nearest bf16 (ties to even) as fp32; finite inputs"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def one_hot_rows(rng, K, n):
    """[K x n]: column j holds 2^e_j at row k_j and zeros elsewhere; the k_j walk every row of K when n >= K, and the last and the first
    row of K are among them"""
    k = np.arange(n) % K if n >= K else rng.randint(0, K, size=n)
    k = rng.permutation(k)
    k[0], k[-1] = K - 1, 0
    w = np.exp2(rng.randint(-8, 9, size=n)).astype(np.float32)
    m = np.zeros((K, n), np.float32)
    m[k, np.arange(n)] = w
    return m, k, w


@functools.lru_cache(maxsize=None)
def exact_case(M, N, K, side, nprod):
    """operands and the exact result; shared between tests: read only"""
    rng = np.random.RandomState(M + 3 * N + 7 * K + 11 * nprod + (side == 'B'))
    rnd = full_mantissa(rng, K, M if side == 'A' else N)
    if nprod == 1:
        rnd = to_bf16(rnd)
    if side == 'A':
        A = rnd
        B, k, w = one_hot_rows(rng, K, N)
        ref = A[k, :].T * w[None, :]
    else:
        B = rnd
        A, k, w = one_hot_rows(rng, K, M)
        ref = B[k, :] * w[:, None]
    assert np.array_equal(ref.astype(np.float64), A.astype(np.float64).T @ B.astype(np.float64))   # the fp64 product, exactly
    return A, B, ref


def run(split_tn, A, B, out, nprod, launches=1):
    K, M = A.shape
    N = B.shape[1]
    Ad, Bd = tog.dev(A), tog.dev(B)
    for _ in range(launches):
        split_tn(ptr(Ad), M, ptr(Bd), N, ptr(out.t), N, M, N, K, nprod, stream())
    torch.cuda.synchronize()
    return out.t.cpu().numpy()


@pytest.mark.parametrize("nprod", [9, 1])
@pytest.mark.parametrize("side", ['A', 'B'])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_contraction_exact(split_tn, M, N, K, side, nprod):
    """C = A^T B from zero, bit for bit; side B: the shared tile is the random operand -- different in every column tile and every k"""
    A, B, ref = exact_case(M, N, K, side, nprod)
    out = ar.Guarded((M, N), init=np.zeros((M, N), np.float32))
    got = run(split_tn, A, B, out, nprod)
    assert np.array_equal(got, ref), 'nprod %d side %s (%d, %d, %d): %s' % (nprod, side, M, N, K, first_difference(got, ref))
    assert not out.written_guard_rows()


@pytest.mark.parametrize("nprod", [9, 1])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_two_launches_into_one_sum(split_tn, M, N, K, nprod):
    """two launches back to back into the same C: exactly twice one launch's result"""
    A, B, ref = exact_case(M, N, K, 'B', nprod)
    out = ar.Guarded((M, N), init=np.zeros((M, N), np.float32))
    got = run(split_tn, A, B, out, nprod, launches=2)
    assert np.array_equal(got, ref + ref), 'nprod %d (%d, %d, %d): %s' % (nprod, M, N, K, first_difference(got, ref + ref))
    assert not out.written_guard_rows()


@pytest.mark.parametrize("nprod", [9, 1])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_contraction_random(split_tn, M, N, K, nprod):
    """both operands random full-mantissa, accumulated onto a non-zero C; rel-L2 of the added sum against fp64"""
    rng = np.random.RandomState(5 * M + 3 * N + K + nprod)
    A, B = full_mantissa(rng, K, M), full_mantissa(rng, K, N)
    if nprod == 9:
        ref = A.astype(np.float64).T @ B.astype(np.float64)
    else:
        ref = to_bf16(A).astype(np.float64).T @ to_bf16(B).astype(np.float64)
    C0 = acc_init(rng, ref)
    out = ar.Guarded((M, N), init=C0)
    got = run(split_tn, A, B, out, nprod).astype(np.float64)
    err = np.linalg.norm(got - (C0.astype(np.float64) + ref)) / np.linalg.norm(ref)
    bound = min(12 * np.sqrt(K) * 2.0 ** -24, 2e-5)
    print('nprod %d (%d, %d, %d): rel-L2 %.3e, bound %.3e' % (nprod, M, N, K, err, bound))
    assert err < bound
    assert not out.written_guard_rows()
