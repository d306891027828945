"""The residual-flagging cases worked by hand, shared by tests/test_flag_host.py (the restatement against the hand result)
and tests/test_gpu_flag.py (the device against the restatement).  Every case is one group of real amplitudes (vis = a + 0j,
no model): name -> (amplitudes, keyword arguments, the expected codes, { n, med, MAD, T } of the last round that ran,
the expected 8 stats)."""
import numpy as np

INF, NAN = np.inf, np.nan


def T(med, nsigma, mad):
    """the header's expression, each operation rounded once"""
    return np.float64(med) + np.float64(nsigma) * (np.float64(1.4826) * np.float64(mad))


HAND = {
    # med = 5 (rank 4 of 9), d = 4 3 2 1 0 1 2 3 95 -> MAD 2, T = 5 + 5 * 2.9652 = 19.826: 100 goes.  Round 1 over 1 .. 8:
    # med = 4 (rank 3 of 8, the LOWER median), d = 3 2 1 0 1 2 3 4 -> MAD 2, T = 18.826: nothing goes, the loop stops.
    "nine_one_outlier": ([1, 2, 3, 4, 5, 6, 7, 8, 100], dict(nsigma=5.0, min_count=8, niter=3),
                         [0] * 8 + [16], (8, 4.0, 2.0, T(4, 5, 2)), [2, 9, 1, 0, 0, 0, 0, 8]),
    # an even count: the lower median of 1 2 3 4 is 2, not 2.5; d = 1 0 1 2 -> the lower median of 0 1 1 2 is 1
    "even_count": ([4, 1, 3, 2], dict(nsigma=5.0, min_count=1, niter=1),
                   [0] * 4, (4, 2.0, 1.0, T(2, 5, 1)), [1, 4, 0, 0, 0, 0, 0, 4]),
    # all ties: MAD = 0, so sigma = 0 and T = +Inf whatever nsigma is
    "all_ties": ([3.5] * 10, dict(nsigma=0.001, min_count=1, niter=4),
                 [0] * 10, (10, 3.5, 0.0, INF), [1, 10, 0, 0, 0, 0, 0, 10]),
    # five samples with min_count = 8: the statistics are reported, T = +Inf, the gross outlier stays
    "below_min_count": ([1, 2, 3, 4, 1e6], dict(nsigma=3.0, min_count=8, niter=3),
                        [0] * 5, (5, 3.0, 1.0, INF), [1, 5, 0, 0, 0, 0, 0, 5]),
    # round 0: med 10, d = 10 9 8 7 0 1 2 30 990 -> MAD 8, T = 10 + 3 * 11.8608 = 45.58: 1000 goes, 40 stays.
    # round 1 over 8: med 3 (rank 3), d = 3 2 1 0 7 8 9 37 -> MAD 3, T = 3 + 3 * 4.4478 = 16.34: 40 goes.
    # round 2 over 7: med 3, MAD 3, the same T: 12 stays, the loop stops - 3 rounds run.
    "two_rounds": ([0, 1, 2, 3, 10, 11, 12, 40, 1000], dict(nsigma=3.0, min_count=4, niter=8),
                   [0] * 7 + [17, 16], (7, 3.0, 3.0, T(3, 3, 3)), [3, 9, 2, 0, 0, 0, 0, 7]),
}


def hand(name):
    a, kw, codes, gstats, stats = HAND[name]
    return (np.array(a, dtype=np.float64).astype(np.complex128), kw, np.array(codes, dtype=np.uint8),
            np.array([gstats], dtype=np.float64), np.array(stats, dtype=np.float64))
