"""The CPU restatement of the particle filter's noise stream (tests/noise_restatement.py) held to
what does not depend on it: the published Random123 known answers, counters whose words were
searched for once, and the float32 facts of the uniform."""
import numpy as np
import pytest

import noise_restatement as R

KAT, KAT_STREAM = R.KAT, R.KAT_STREAM
DESIGNED_SEED, DESIGNED_STEP, DESIGNED, R_MAX = R.DESIGNED_SEED, R.DESIGNED_STEP, R.DESIGNED, R.R_MAX


def test_philox_known_answers():
    for ctr, key, out in KAT:
        got = R.philox4x32_10(np.array([ctr], dtype=np.uint64), np.array([key], dtype=np.uint64))[0]
        assert [int(v) for v in got] == list(out)


def test_philox_words_put_index_step_and_seed_where_the_header_says():
    """counter = (index lo, index hi, step lo, step hi), key = (seed lo, seed hi): the known
    answers again, through the 64-bit arguments."""
    for (seed, step, first), (_, _, out) in zip(KAT_STREAM, KAT):
        assert [int(v) for v in R.philox_words(seed, step, first, 1)[0]] == list(out)
    # a run of indices is one counter per particle, also across a carry into the high word
    first = (1 << 32) - 2
    run = R.philox_words(7, 9, first, 4)
    for j in range(4):
        i = first + j
        one = R.philox4x32_10(np.array([[i & 0xffffffff, i >> 32, 9, 0]], dtype=np.uint64),
                              np.array([[7, 0]], dtype=np.uint64))[0]
        assert np.array_equal(run[j], one)


@pytest.mark.parametrize("index,word,value", DESIGNED)
def test_designed_counters_have_their_words(index, word, value):
    w = R.philox_words(DESIGNED_SEED, DESIGNED_STEP, index, 1)[0]
    assert int(w[word]) == value
    assert (value >> 8) in (0, 0xffffff)


def test_designed_counters_give_the_ends_of_the_stream():
    z, r = R.normals_reference(DESIGNED_SEED, DESIGNED_STEP, R.D_UR_ONE, 1)
    assert r[0, 0] == 0.0 and z[0, 0] == 0.0 and z[0, 1] == 0.0 and np.isfinite(z).all()
    z, r = R.normals_reference(DESIGNED_SEED, DESIGNED_STEP, R.D_UR2_ONE, 1)
    assert r[0, 2] == 0.0 and z[0, 2] == 0.0 and np.isfinite(z).all()
    _, r = R.normals_reference(DESIGNED_SEED, DESIGNED_STEP, R.D_UR_MIN, 1)
    assert r[0, 0] == pytest.approx(R_MAX, rel=1e-15, abs=0) and abs(R_MAX - 5.8870501) < 1e-7
    _, r = R.normals_reference(DESIGNED_SEED, DESIGNED_STEP, R.D_UR2_MIN, 1)
    assert r[0, 2] == pytest.approx(R_MAX, rel=1e-15, abs=0)


def test_unit_f32_facts():
    def u(k):
        return R.unit_f32(np.uint64(k) << np.uint64(8))

    for k in (0, 1, 2 ** 23 - 1):                      # below 2^23 the sum is exact
        assert float(u(k)) == (k + 0.5) / 2.0 ** 24
    assert u(0).dtype == np.float32
    assert float(u(2 ** 23)) == 0.5                    # 2^23 + 0.5 ties to even: 2^23
    assert float(u(2 ** 23 + 1)) == (2 ** 23 + 2) / 2.0 ** 24      # odd k rounds up
    assert float(u(2 ** 24 - 1)) == 1.0
    # the low 8 bits of the word do not matter
    assert float(R.unit_f32(0xffffffff)) == 1.0 and float(R.unit_f32(0xff)) == 2.0 ** -25
    k = np.unique(np.concatenate([np.arange(0, 2 ** 24, 37), np.arange(2 ** 23 - 4096, 2 ** 23 + 4096),
                                  np.arange(4096), np.arange(2 ** 24 - 4096, 2 ** 24)])).astype(np.uint64)
    v = R.unit_f32(k << np.uint64(8))
    assert v.dtype == np.float32 and v.min() == np.float32(2.0 ** -25) and v.max() == np.float32(1.0)
    assert (v > 0).all() and (v <= 1).all()
    # never farther than the float32 rounding of k + 0.5 (half an ulp of 2^24: 0.5) from the ideal
    ideal = (k.astype(np.float64) + 0.5) / 2.0 ** 24
    assert np.max(np.abs(v.astype(np.float64) - ideal)) == 2.0 ** -25
    assert np.array_equal(v[k < 2 ** 23].astype(np.float64), ideal[k < 2 ** 23])


def test_normals_reference_is_a_standard_normal_stream():
    """A sanity check of the restatement's own arithmetic (Box-Muller over the words)."""
    n = 200000
    z, r = R.normals_reference(2024, 1, 0, n)
    assert z.shape == (n, 3) and r.shape == (n, 3) and z.dtype == np.float64
    assert np.isfinite(z).all() and np.all(np.abs(z) <= r)
    se = 1.0 / np.sqrt(n)
    assert np.all(np.abs(z.mean(axis=0)) < 5 * se)
    assert np.all(np.abs(z.var(axis=0) - 1.0) < 5 * np.sqrt(2.0) * se)
    assert np.all(np.abs(np.corrcoef(z.T) - np.eye(3)) < 5 * se)
    # shard invariance: a sub-range is the slice
    part, _ = R.normals_reference(2024, 1, 4097, 100)
    assert np.array_equal(part, z[4097:4197])
