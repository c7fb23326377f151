"""tests/_gemv_oracle.py, the skinny GEMM's arithmetic restated in numpy float32, against the real
dot product in fp64 under the bound derived there, and its own structure: the lane order, the fold,
the epilogues' single rounding, and that a row's sum does not depend on the other rows."""
import numpy as np
import pytest

import _gemv_oracle as O

SHAPES = [(1, 24, 64), (5, 23, 4104), (2, 7, 4608), (3, 10, 8192), (8, 16, 6400), (3, 9, 3072), (4, 5, 520)]


def _bf16(rng, *shape, scale=1.0):
    """Random float32 values that are bf16 values."""
    return O.bf16_round((rng.standard_normal(shape) * scale).astype(np.float32))[1]


@pytest.mark.parametrize("B,N,K", SHAPES, ids=lambda v: str(v))
def test_within_bound_of_the_real_dot_product(B, N, K):
    rng = np.random.default_rng(K + B)
    x, w = _bf16(rng, B, K), _bf16(rng, N, K, scale=0.05)
    _, y = O.gemv(x, w, 0)
    ref, tol = O.bound(x, w)
    err = np.abs(y.astype(np.float64) - ref)
    print(f"worst error {float((err / tol).max()):.3f} of the allowed")
    assert (err <= tol).all()


@pytest.mark.parametrize("B,N,K", [(1, 24, 64), (2, 7, 8), (8, 9, 1032), (5, 10, 4096), (3, 9, 3072), (4, 5, 520)],
                         ids=lambda v: str(v))
def test_wide_restatement_within_bound_of_the_real_dot_product(B, N, K):
    """The wide path's 16 lanes per column (K <= 4096 there), under the bound at L = 16."""
    rng = np.random.default_rng(K + B)
    x, w = _bf16(rng, B, K), _bf16(rng, N, K, scale=0.05)
    _, y = O.gemv(x, w, 0, lanes=O.WIDE_LANES)
    ref, tol = O.bound(x, w, O.WIDE_LANES)
    err = np.abs(y.astype(np.float64) - ref)
    print(f"worst error {float((err / tol).max()):.3f} of the allowed")
    assert (err <= tol).all()


def test_epilogues_add_in_fp32_and_round_once():
    """Bias and residual enter as single fp32 adds after the fold: two more roundings to half an ulp
    of a value that |dot| + |bias| + |resid| bounds, doubled, on top of the dot product's bound."""
    rng = np.random.default_rng(3)
    B, N, K = 3, 12, 5120
    x, w = _bf16(rng, B, K), _bf16(rng, N, K, scale=0.05)
    bias, resid = _bf16(rng, N), _bf16(rng, B, N)
    ref, tol = O.bound(x, w)
    mass = np.abs(ref) + np.abs(bias)[None] + np.abs(resid)
    for epi, want in ((1, ref + bias[None]), (3, ref + bias[None] + resid)):
        _, y = O.gemv(x, w, epi, bias, resid)
        allowed = tol + 2.0 ** -8 * (np.abs(want) - np.abs(ref)).clip(min=0) + 4 * 2.0 ** -24 * mass
        assert (np.abs(y - want) <= allowed).all()
    z = (ref + bias[None])
    want = 0.5 * z * (1 + np.tanh(0.7978845608028654 * (z + 0.044715 * z ** 3)))
    np.testing.assert_allclose(O.gemv(x, w, 2, bias)[1], want, atol=2e-2, rtol=2e-2)


def test_lane_and_chunk_order():
    """Column c belongs to lane (c % 512) // 8; a lane adds its elements in column order, round after
    round.  1, 2^24 and -2^24 in one lane sum to 0 or 1 in fp32 depending on the order alone."""
    K = 1024
    w = np.ones((1, K), dtype=np.float32)
    x = np.zeros((1, K), dtype=np.float32)
    x[0, 8 * 5 + 3] = 7.0
    x[0, 512 + 8 * 5] = 11.0
    x[0, 8 * 9] = 13.0
    acc = O.lane_sums(x, w)[0, 0]
    assert acc[5] == 18.0 and acc[9] == 13.0 and acc.sum() == 31.0
    x[:] = 0.0
    x[0, [16, 17, 512 + 16]] = [1.0, 2.0 ** 24, -2.0 ** 24]  # lane 2: (1 + 2^24) - 2^24 = 0 in fp32
    assert O.lane_sums(x, w)[0, 0, 2] == 0.0
    x[0, [16, 17, 512 + 16]] = [2.0 ** 24, -2.0 ** 24, 1.0]
    assert O.lane_sums(x, w)[0, 0, 2] == 1.0


def test_wide_lane_and_chunk_order():
    """16 lanes: column c belongs to lane (c % 128) // 8, rounds of 128 columns in ascending order
    across the 1024-column segments; the fold is the xor tree over 1, 2, 4, 8."""
    K = 2048
    w = np.ones((1, K), dtype=np.float32)
    x = np.zeros((1, K), dtype=np.float32)
    x[0, 8 * 5 + 3] = 7.0
    x[0, 128 + 8 * 5] = 11.0
    x[0, 1024 + 8 * 5 + 1] = 17.0
    x[0, 8 * 9] = 13.0
    acc = O.lane_sums(x, w, 16)[0, 0]
    assert acc.shape == (16,) and acc[5] == 35.0 and acc[9] == 13.0 and acc.sum() == 48.0
    x[:] = 0.0
    x[0, [16, 17, 1024 + 16]] = [1.0, 2.0 ** 24, -2.0 ** 24]  # lane 2, across a segment: (1 + 2^24) - 2^24 = 0
    assert O.lane_sums(x, w, 16)[0, 0, 2] == 0.0
    x[0, [16, 17, 1024 + 16]] = [2.0 ** 24, -2.0 ** 24, 1.0]
    assert O.lane_sums(x, w, 16)[0, 0, 2] == 1.0
    acc = np.zeros((1, 1, 16), dtype=np.float32)
    acc[0, 0, :4] = [2.0 ** 24, 1.0, 1.0, -2.0 ** 24]  # pairs first: (2^24 + 1 -> 2^24) + (1 - 2^24) = 1
    assert O.fold(acc, 16)[0, 0] == 1.0
    rng = np.random.default_rng(1)
    a = rng.standard_normal((2, 3, 16)).astype(np.float32)
    s = a.copy()
    for o in (1, 2, 4, 8):
        s = np.stack([s[..., j] + s[..., j ^ o] for j in range(16)], axis=-1)
    assert (s == s[..., :1]).all() and np.array_equal(O.fold(a, 16), s[..., 0])


def test_fold_is_the_xor_tree():
    """Lane 0 ends with ((l0 + l1) + (l2 + l3)) + ...: pairs first, not a running sum."""
    acc = np.zeros((1, 1, 64), dtype=np.float32)
    acc[0, 0, :4] = [2.0 ** 24, 1.0, 1.0, -2.0 ** 24]  # pairs: (2^24 + 1 -> 2^24) + (1 - 2^24) = 1
    assert O.fold(acc)[0, 0] == 1.0
    acc[0, 0, :4] = [1.0, 1.0, 2.0 ** 24, -2.0 ** 24]  # (1 + 1) + 0
    assert O.fold(acc)[0, 0] == 2.0
    rng = np.random.default_rng(0)
    a = rng.standard_normal((2, 3, 64)).astype(np.float32)
    s = a.copy()
    for o in (1, 2, 4, 8, 16, 32):
        s = np.stack([s[..., j] + s[..., j ^ o] for j in range(64)], axis=-1)
    assert (s == s[..., :1]).all() and np.array_equal(O.fold(a), s[..., 0])


def test_rows_are_independent():
    rng = np.random.default_rng(5)
    x, w = _bf16(rng, 8, 4104), _bf16(rng, 9, 4104, scale=0.05)
    bits, _ = O.gemv(x, w, 0)
    for b in (0, 3, 7):
        assert np.array_equal(O.gemv(x[b:b + 1], w, 0)[0][0], bits[b])


def test_bf16_rounding_is_nearest_even():
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0], dtype=np.float32)
    bits, back = O.bf16_round(v)
    assert back.tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0]
    assert bits[0] == 0x3F80 and bits[4] == 0xC040
