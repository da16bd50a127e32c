"""The law of sxmc_sample_multiplicities (include/sxmc_hip.h) restated in numpy: real Monte Carlo sample weights as
integer multiplicities on a power-of-two scale.  TEST INFRASTRUCTURE: what the library's one implementation
(sxmc_amd/csrc/sample_multiplicities.h) is held to, as bytes.

    m_i = (unsigned) nearbyint(ldexp(w_i, k)), half to even;
    k = the largest integer in [-32, 24] with every m_i <= 2^32 - 1 and sum m_i <= max_total (0 means 2^32 - 1);
    refused: max_total > 2^32 - 1, a weight that is negative or not finite (the first such row is named), no such k,
    a total of 0 at the chosen k.
"""
import numpy as np

MAX_TOTAL = 2**32 - 1
K_MIN, K_MAX = -32, 24


class Refused(Exception):
    def __init__(self, why, row=None):
        super().__init__(why if row is None else "%s (row %d)" % (why, row))
        self.why, self.row = why, row


def sample_multiplicities(w, max_total=0):
    """(m uint32 [n], k, total) or raises Refused."""
    w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
    max_total = int(max_total) or MAX_TOTAL
    if max_total > MAX_TOTAL:
        raise Refused("max_total")
    bad = np.flatnonzero(~(w >= 0.0) | np.isinf(w))
    if bad.size:
        raise Refused("weight", int(bad[0]))
    for k in range(K_MAX, K_MIN - 1, -1):
        with np.errstate(over="ignore"):
            r = np.rint(np.ldexp(w, k))              # (rint: half to even, as nearbyint in the default rounding mode)
        if r.size and r.max() > float(MAX_TOTAL):
            continue
        total = int(r.astype(np.uint64).sum())       # exact: fewer than 2^32 rows of at most 2^32 - 1 each
        if total > max_total:
            continue
        if total == 0:
            raise Refused("zero total")
        return r.astype(np.uint32), k, total
    raise Refused("no scale")
