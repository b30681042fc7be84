"""
motifscan_amd.dimodel -- first-order motif models: the score of a column depends on the base of the column before it (dinucleotide
weight matrices, first-order BaMMs, TFFMs).  A PWM cannot tell TGACGTCA / TGAGCTCA from TGACCTCA / TGAGGTCA; a first-order model can.
include/motifscan_amd.h has the definition the device follows (ms_scan_best_dimodels, ms_dimodel.hip); this module holds the model, the
ways to build one, and the definition restated in numpy.

    DiModel(start, trans)             start float64 [4]; trans float64 [W - 1][16]: trans[j - 1][4 a + b] scores base b at column j
                                      given base a at column j - 1 (the header's trans[j], j = 1 .. W - 1).  .width, .values()
    DiModel.from_pwm(matrix)          the degenerate model of a PWM [4][W]: the same raw sums as the PWM on both strands, bit for bit
    DiModel.from_counts(first, pairs, cond, init, pseudocount=1.0)
                                      log-odds of observed counts against an order-1 background
    DiModel.from_site_stack(stack, i, cond, init, pseudocount=1.0)
                                      ... of the counts of row i of a sitestack.SiteStack made with dinuc=True
    DiModelSet(models)                a list of models with the arrays the library reads (.values, .widths)
    max_raw_host(model)               the Viterbi maximum, in the header's arithmetic
    scorable_host(model)              the header's test for a model that is scored at all
    window_sums_host(model, seq)      (forward, reverse) raw sums of every window start, NaN where the window holds a non-ACGT base
    best_sites_host(models, sequences, strand)
                                      (score, pos, strand) planes [P][R] as ms_scan_best_dimodels defines them: the same additions in
                                      the same order, so the device's planes equal these byte for byte

The device side is _lib.DiModelSet / _lib.scan_best_dimodels and Scanner.best_sites_dimodels / rank_sum_dimodels; there is no CPU path
behind those.
"""
import numpy as np

_STRAND_FLAG = {"+": 1, "-": 2, "both": 3}

# ASCII -> 0 .. 3 for A, C, G, T in either case, -1 for every other byte (as the library's packer reads a base)
_CODE = np.full(256, -1, dtype=np.int8)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _i


class DiModel:
    """One first-order model: start [4] and trans [W - 1][16] of float64 (a model of one column has no trans rows)."""
    __slots__ = ("start", "trans")

    def __init__(self, start, trans):
        self.start = np.array(start, dtype=np.float64)
        trans = np.array(trans, dtype=np.float64)
        self.trans = trans.reshape(0, 16) if trans.size == 0 else trans
        if self.start.shape != (4,):
            raise ValueError(f"start must hold 4 values, got shape {self.start.shape}")
        if self.trans.ndim != 2 or self.trans.shape[1] != 16:
            raise ValueError(f"trans must be [W - 1][16], got shape {self.trans.shape}")

    @property
    def width(self):
        return self.trans.shape[0] + 1

    def values(self):
        """float64 [W][16] as the library takes a model: row 0 = start in its first four entries (the other twelve 0.0, never read),
        row j >= 1 = trans[j - 1]."""
        out = np.zeros((self.width, 16), dtype=np.float64)
        out[0, :4] = self.start
        out[1:] = self.trans
        return out

    @classmethod
    def from_pwm(cls, matrix):
        """start[b] = M[b][0], trans[j][4 a + b] = M[b][j]: a first-order model that ignores the neighbour."""
        m = np.asarray(matrix, dtype=np.float64)
        if m.ndim != 2 or m.shape[0] != 4 or m.shape[1] < 1:
            raise ValueError("a PWM must be [4][W] with W >= 1")
        return cls(m[:, 0], np.tile(m[:, 1:].T, (1, 4)))

    @classmethod
    def from_counts(cls, first, pairs, cond, init, pseudocount=1.0):
        """first [4]: the sites' base counts at column 0; pairs [W - 1][16]: pairs[j - 1][4 a + b] the sites with a at column j - 1 and b
        at column j; cond [4][4] and init [4]: the order-1 background P(b | a) and P(b) (kmers.KmerCounts.markov() of k = 2 and k = 1).
            start[b]          = ln(((first[b] + pc) / (sum first + 4 pc)) / init[b])
            trans[j][4 a + b] = ln(((pairs[j - 1][4 a + b] + pc) / (sum over b' of pairs[j - 1][4 a + b'] + 4 pc)) / cond[a][b])
        rounded to 5 decimals, as matrix.columns_to_pwm rounds a PWM."""
        pc = float(pseudocount)
        if not pc > 0:
            raise ValueError("pseudocount must be > 0")
        first = np.asarray(first, dtype=np.float64)
        pairs = np.asarray(pairs, dtype=np.float64)
        pairs = pairs.reshape(0, 16) if pairs.size == 0 else pairs
        cond = np.asarray(cond, dtype=np.float64)
        init = np.asarray(init, dtype=np.float64).reshape(-1)
        if first.shape != (4,) or pairs.ndim != 2 or pairs.shape[1] != 16 or cond.shape != (4, 4) or init.shape != (4,):
            raise ValueError("need first[4], pairs[W - 1][16], cond[4][4] and init[4]")
        if (first < 0).any() or (pairs < 0).any() or not (cond > 0).all() or not (init > 0).all():
            raise ValueError("counts must be >= 0 and background probabilities > 0")
        start = np.around(np.log(((first + pc) / (first.sum() + 4 * pc)) / init), 5)
        p = pairs.reshape(-1, 4, 4)
        trans = np.around(np.log(((p + pc) / (p.sum(axis=2, keepdims=True) + 4 * pc)) / cond[None, :, :]), 5)
        return cls(start, trans.reshape(-1, 16))

    @classmethod
    def from_site_stack(cls, stack, i, cond, init, pseudocount=1.0):
        """from_counts of row i of a SiteStack (sitestack.site_base_counts(..., dinuc=True)): first = counts[i][flank][0:4], pairs[j] =
        dinuc[i][flank + j] for j = 0 .. W - 2."""
        if stack.dinuc is None:
            raise ValueError("the site stack holds no pair counts: make it with dinuc=True")
        W, flank = int(stack.widths[i]), int(stack.flank)
        return cls.from_counts(stack.counts[i][flank][0:4], stack.dinuc[i][flank:flank + W - 1], cond, init, pseudocount)


class DiModelSet:
    """A list of DiModel with the arrays ms_dimodelset_create reads: values float64 [sum of W][16], widths int32 [P]."""

    def __init__(self, models):
        self.models = list(models)
        for m in self.models:
            if not isinstance(m, DiModel):
                raise TypeError("a DiModelSet holds DiModel objects")
        self.widths = np.array([m.width for m in self.models], dtype=np.int32)
        self.values = np.concatenate([m.values() for m in self.models]) if self.models else np.zeros((0, 16), dtype=np.float64)

    def __len__(self):
        return len(self.models)

    def __getitem__(self, i):
        return self.models[i]

    def __iter__(self):
        return iter(self.models)


def _models(models):
    if isinstance(models, DiModelSet):
        return models.models
    if isinstance(models, DiModel):
        return [models]
    return list(models)


def max_raw_host(model):
    """v_0 = start; v_j[b] = max over a of (v_{j-1}[a] + trans[j][4 a + b]); the greatest entry of the last v."""
    v = model.start.copy()
    with np.errstate(invalid="ignore"):
        for t in model.trans:
            v = np.max(v[:, None] + t.reshape(4, 4), axis=0)
    return float(np.max(v))


def scorable_host(model):
    """max_raw is a finite number > 0 and no entry is NaN or +inf (-inf is allowed: a forbidden transition)."""
    mr = max_raw_host(model)
    entries = np.concatenate([model.start, model.trans.ravel()])
    return bool(np.isfinite(mr) and mr > 0.0 and not np.isnan(entries).any() and not (entries == np.inf).any())


def _codes(seq):
    raw = seq.encode("latin-1", "replace") if isinstance(seq, str) else bytes(seq)
    return _CODE[np.frombuffer(raw, dtype=np.uint8)].astype(np.int64)


def window_sums_host(model, seq):
    """(fwd, rev) float64 [max(L - W + 1, 0)]: the raw sums of every window start of `seq` in the header's order of additions; NaN for
    a window that holds a non-ACGT base."""
    x = _codes(seq)
    W, n = model.width, len(x) - model.width + 1
    if n <= 0:
        return np.zeros(0), np.zeros(0)
    non = np.concatenate([[0], np.cumsum(x < 0)])
    valid = non[W:] - non[:-W] == 0
    xs = np.where(x < 0, 0, x)
    fwd = np.zeros(n) + model.start[xs[:n]]
    rev = np.zeros(n)
    for c in range(1, W):
        a, b = xs[c - 1:c - 1 + n], xs[c:c + n]
        fwd = fwd + model.trans[c - 1][4 * a + b]
        rev = rev + model.trans[W - c - 1][4 * (3 - b) + (3 - a)]
    rev = rev + model.start[3 - xs[W - 1:W - 1 + n]]
    return np.where(valid, fwd, np.nan), np.where(valid, rev, np.nan)


def best_sites_host(models, sequences, strand=3):
    """ms_scan_best_dimodels restated: (score float64, pos int32, strand int8) [P][R].  strand: 1, 2, 3 or '+', '-', 'both'."""
    mask = _STRAND_FLAG.get(strand, strand)
    if mask not in (1, 2, 3):
        raise ValueError(f"invalid strand mask {strand!r} (1 '+', 2 '-', 3 both)")
    models, sequences = _models(models), list(sequences)
    shape = (len(models), len(sequences))
    score, pos, strd = np.full(shape, np.nan), np.full(shape, -1, dtype=np.int32), np.zeros(shape, dtype=np.int8)
    for i, m in enumerate(models):
        if not scorable_host(m):
            continue
        max_raw = max_raw_host(m)
        for r, s in enumerate(sequences):
            fwd, rev = window_sums_host(m, s)
            if not len(fwd):
                continue
            q = np.stack([fwd if mask & 1 else np.full(len(fwd), np.nan), rev if mask & 2 else np.full(len(rev), np.nan)], axis=1) / max_raw
            q = np.where(np.isnan(q), -np.inf, q).ravel()         # pos ascending, '+' before '-': the first maximum is the walk's winner
            k = int(np.argmax(q))
            if q[k] > -np.inf:
                score[i, r], pos[i, r], strd[i, r] = q[k], k >> 1, 1 + (k & 1)
    return score, pos, strd
