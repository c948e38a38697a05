"""The particle filter's noise stream (include/ndt2d_hip.h, "particle-filter steps either side of
`measure`"; csrc/ndt2d_motion.hip) restated on the CPU in numpy.  Test infrastructure only: the
yardstick of tests/test_noise_restatement.py (which pins it to the Random123 known answers) and of
the noise tests in tests/test_gpu_particle_filter.py; tests/test_gpu_resample.py takes its Philox
from here as well.

The stream of particle `index` at (seed, step):
    w[0..3] = Philox4x32-10(counter = (index lo, index hi, step lo, step hi), key = (seed lo, seed hi))
    u(w)    = float32 round-to-nearest-even of ((w >> 8) + 0.5), times 2^-24        in (0, 1]
    r0 = sqrt(-2 log u(w0)),  r1 = sqrt(-2 log u(w2))
    a0 = float32(2 pi) * u(w1),  a1 = float32(2 pi) * u(w3)       (float32 products)
    z  = (r0 cos a0, r0 sin a0, r1 cos a1)
The uniforms and the angles are float32 values that IEEE arithmetic fixes to the bit, so they are
computed here in float32 and belong to the stream's definition; log, sqrt, cos and sin are taken
in float64 (about 2^29 times finer than the float32 results they judge).
"""
import numpy as np

_M32 = np.uint64(0xffffffff)
_S32 = np.uint64(32)
TWO_PI_F32 = np.float32(6.28318530717958647692)

# Random123's kat_vectors for philox4x32-10: (counter, key, output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
# The same three as (seed, step, first index) of the noise stream
KAT_STREAM = [(0, 0, 0), ((1 << 64) - 1,) * 3,
              (0x299f31d0a4093822, 0x0370734413198a2e, 0x85a308d3243f6a88)]

# seed = 1, step = 1: the particle indices whose words have all-ones / all-zero top 24 bits, i.e.
# the ends of the uniform (found by a search over indices 0 .. 2^25; tests/test_noise_restatement.py
# asserts the words): (index, word number, word)
DESIGNED_SEED, DESIGNED_STEP = 1, 1
D_UR_ONE, D_UR_MIN, D_UR2_ONE, D_UR2_MIN, D_UA_ONE, D_UA_MIN = (
    25324145, 6983761, 13862772, 19050278, 9474925, 27077537)
DESIGNED = [(D_UR_ONE, 0, 0xffffffdf),    # u_r == 1.0f: r0 = 0, z0 = z1 = 0
            (D_UR_MIN, 0, 0x0000001c),    # u_r = 2^-25: r0 = sqrt(50 ln 2) = 5.887..., the largest
            (D_UR2_ONE, 2, 0xffffffc8),   # r1 = 0: z2 = 0
            (D_UR2_MIN, 2, 0x000000db),   # the largest r1
            (D_UA_ONE, 1, 0xffffff64),    # angle = float32 2 pi
            (D_UA_MIN, 1, 0x00000021)]    # the smallest angle, 2 pi 2^-25
R_MAX = float(np.sqrt(50.0 * np.log(2.0)))    # sqrt(-2 log 2^-25) = 5.8870501...


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64-held 32-bit words: counter [..., 4],
    key [..., 2] -> [..., 4]."""
    m32 = _M32
    c = [np.asarray(counter[..., k], dtype=np.uint64) for k in range(4)]
    k0 = np.asarray(key[..., 0], dtype=np.uint64)
    k1 = np.asarray(key[..., 1], dtype=np.uint64)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, axis=-1)


def philox_words(seed, step, first, n):
    """The four 32-bit words (uint64-held, [n, 4]) of particles first .. first + n: counter =
    (index lo, index hi, step lo, step hi), key = (seed lo, seed hi); the index wraps at 2^64."""
    seed, step, first = int(seed), int(step), int(first)
    with np.errstate(over="ignore"):
        i = np.uint64(first) + np.arange(n, dtype=np.uint64)
    ctr = np.stack([i & _M32, i >> _S32, np.full(n, step & 0xffffffff, dtype=np.uint64),
                    np.full(n, step >> 32, dtype=np.uint64)], axis=-1)
    key = np.stack([np.full(n, seed & 0xffffffff, dtype=np.uint64),
                    np.full(n, seed >> 32, dtype=np.uint64)], axis=-1)
    return philox4x32_10(ctr, key)


def unit_f32(word):
    """The stream's uniform of a 32-bit word, in float32 arithmetic: fl(k + 0.5) * 2^-24 with
    k = word >> 8.  k + 0.5 needs 25 significand bits from k = 2^23, so there the sum is rounded
    to even (k even: k, k odd: k + 1) and k = 2^24 - 1 gives 1.0; the product is exact."""
    k = (np.asarray(word, dtype=np.uint64) >> np.uint64(8)).astype(np.float32)   # k < 2^24: exact
    return (k + np.float32(0.5)) * np.float32(2.0 ** -24)


def normals_reference(seed, step, first, n):
    """(z [n, 3], r [n, 3]) in float64: the three standard normals of every particle and, for each
    of them, the Box-Muller radius it was made with (r0, r0, r1)."""
    w = philox_words(seed, step, first, n)
    u_r = np.stack([unit_f32(w[:, 0]), unit_f32(w[:, 2])], axis=-1)
    u_a = np.stack([unit_f32(w[:, 1]), unit_f32(w[:, 3])], axis=-1)
    assert u_r.dtype == np.float32 and u_a.dtype == np.float32
    angle = TWO_PI_F32 * u_a
    assert angle.dtype == np.float32
    r = np.sqrt(-2.0 * np.log(u_r.astype(np.float64)))
    a = angle.astype(np.float64)
    z = np.stack([r[:, 0] * np.cos(a[:, 0]), r[:, 0] * np.sin(a[:, 0]), r[:, 1] * np.cos(a[:, 1])],
                 axis=-1)
    return z, np.stack([r[:, 0], r[:, 0], r[:, 1]], axis=-1)
