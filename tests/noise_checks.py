"""What the noise tests assert, shared by the CPU and the GPU file."""
import numpy as np

import noise_reference as ref

# |M2_32 - M2_64| <= C * u * (n * M2 + n^1.5 * x_max * sqrt(M2) + n * u * x_max^2): Welford's update in float32 against two passes in float64.
# The worst ratio of the left side to the bracket times u, measured over noise_cases.CPU_STREAMS x CPU_COUNTS x CPU_SEEDS (test_noise.py prints it): WORST_SEEN.
# C is fixed at 4 x that, the margin for other seeds.
WORST_SEEN = 0.296   # uniform samples; lognormal 0.209, tight (1000 +- 1e-2) 0.253, fireflies (2 % at 1e4 over 1e-2) 0.033
C = 4 * WORST_SEEN


def m2_bound_terms(samples):
    """For one stream (n + 1,) float32 (sample 0 included): (|M2_32 - M2_64|, u * bracket) with n = the samples past sample 0."""
    x = np.asarray(samples, np.float32)
    n = len(x) - 1
    acc, m2 = np.zeros((1, 4), np.float32), np.zeros((1, 4), np.float32)
    frames = np.zeros((n + 1, 1, 4), np.float32); frames[:, 0, 0] = x
    acc, m2, _ = ref.accumulate(frames, acc, m2, 0)
    _, m2_64 = ref.moments64(x)
    x_max = float(np.abs(x.astype(np.float64)).max())
    bracket = n * m2_64 + n ** 1.5 * x_max * np.sqrt(m2_64) + n * ref.U * x_max ** 2
    return abs(float(m2[0, 0]) - m2_64), ref.U * bracket


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


SENTINEL = 0x7fc0dead   # noise_cases.SENTINEL: the one NaN whose bits do matter


def assert_same_bits(got, want, what):
    """Equal bit for bit. One exception: where both are NaNs that an operation produced (inf - inf in a stream whose M2 has overflowed), any NaN will do -- IEEE 754
    leaves the sign and payload of a generated NaN to the implementation, and the host's differ from the device's. The sentinel's pattern is never excused."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    differ = bits(got) != bits(want)
    differ &= ~(np.isnan(got) & np.isnan(want) & (bits(got) != SENTINEL) & (bits(want) != SENTINEL))
    assert not differ.any(), "%s: %d of %d values differ, first at %s: got %r, want %r" % (
        what, int(differ.sum()), differ.size, tuple(np.argwhere(differ)[0]), got[tuple(np.argwhere(differ)[0])], want[tuple(np.argwhere(differ)[0])])
