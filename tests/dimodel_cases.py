"""
Shared by tests/test_dimodel_host.py and tests/test_gpu_dimodel.py: first-order models and regions at the smallest shapes at which
ms_scan_best_dimodels can go wrong, the definition as a scalar loop (one window, one strand, one addition at a time, in Python floats),
and the planted case of the end-to-end test.  No GPU and no library call in here; the GPU test passes ms_debug_dimodel_dims in.
"""
import itertools

import numpy as np

from motifscan_amd import dimodel

CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}
SMALL_WIDTHS = (1, 2, 3, 31, 32, 33, 34, 63, 64, 65)


def random_dna(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


def random_model(width, seed, holes=0):
    """Log-odds-like entries at five decimals (what from_counts gives); holes: that many transitions (and, from two on, one start entry) set to -inf."""
    rng = np.random.default_rng(seed)
    start = np.round(np.log(rng.dirichlet(np.full(4, 0.6)) / 0.25 + 0.02), 5)
    trans = np.round(np.log(rng.dirichlet(np.full(4, 0.6), size=(width - 1, 4)) / 0.25 + 0.02), 5).reshape(width - 1, 16)
    for _ in range(holes if width > 1 else 0):
        trans[rng.integers(0, width - 1), rng.integers(0, 16)] = -np.inf
    if holes >= 2:
        start[rng.integers(0, 4)] = -np.inf
    return dimodel.DiModel(start, trans)


def random_pwm(width, seed):
    rng = np.random.default_rng(seed)
    ppm = rng.dirichlet(np.full(4, 0.4), size=width).T
    return np.round(np.log2((ppm + 0.01) / 1.04 / 0.25), 5)


def negative_model(width, seed):
    """Every entry < 0: max_raw < 0, unscorable."""
    m = random_model(width, seed)
    return dimodel.DiModel(-np.abs(m.start) - 0.5, -np.abs(m.trans) - 0.5)


def scalar_window(model, seq, p, minus):
    """The raw sum of the window at p on one strand, or None where it holds a non-ACGT base: the header's additions, one at a time."""
    W = model.width
    x = [CODE.get(ch) for ch in seq[p:p + W]]
    if any(b is None for b in x):
        return None
    start, trans = model.start.tolist(), model.trans.tolist()
    s = 0.0
    if not minus:
        s += start[x[0]]
        for j in range(1, W):
            s += trans[j - 1][4 * x[j - 1] + x[j]]
        return s
    y = [3 - x[W - 1 - j] for j in range(W)]
    for j in range(W - 1, 0, -1):
        s += trans[j - 1][4 * y[j - 1] + y[j]]
    s += start[y[0]]
    return s


def scalar_max_raw(model):
    v = model.start.tolist()
    for t in model.trans.tolist():
        v = [max(v[a] + t[4 * a + b] for a in range(4)) for b in range(4)]
    return max(v)


_SUMS = {}                                                # (id(model), seq) -> (model, the windows' scalar sums): the three strand masks share them


def scalar_sums(model, seq):
    key = (id(model), seq)
    if key not in _SUMS:
        _SUMS[key] = (model, [(scalar_window(model, seq, p, False), scalar_window(model, seq, p, True)) for p in range(len(seq) - model.width + 1)])
    return _SUMS[key][1]


def scalar_scorable(model):
    """The header's test, one entry at a time: max_raw a finite number > 0, no entry NaN or +inf."""
    mr = scalar_max_raw(model)
    if mr != mr or mr in (float("inf"), float("-inf")) or not mr > 0.0:
        return False
    return not any(v != v or v == float("inf") for v in model.start.tolist() + model.trans.ravel().tolist())


def scalar_best(model, seq, mask):
    """(score, pos, strand) of one cell by the walk itself: pos ascending, '+' before '-', replace iff greater."""
    if not scalar_scorable(model):
        return np.nan, -1, 0
    max_raw = scalar_max_raw(model)
    best, where = -np.inf, (-1, 0)
    for p, sums in enumerate(scalar_sums(model, seq)):
        for s in (1, 2):
            raw = sums[s - 1]
            if mask & s and raw is not None and raw / max_raw > best:
                best, where = raw / max_raw, (p, s)
    return (best if where[1] else np.nan), where[0], where[1]


def scalar_planes(models, seqs, mask):
    shape = (len(models), len(seqs))
    score, pos, strand = np.full(shape, np.nan), np.full(shape, -1, dtype=np.int32), np.zeros(shape, dtype=np.int8)
    for i, m in enumerate(models):
        for r, s in enumerate(seqs):
            score[i, r], pos[i, r], strand[i, r] = scalar_best(m, s, mask)
    return score, pos, strand


def brute_max_raw(model):
    """The greatest forward raw sum over all 4^W sequences (W small)."""
    return max(scalar_window(model, "".join(t), 0, False) for t in itertools.product("ACGT", repeat=model.width))


def viterbi_sequence(model):
    """A sequence whose forward raw sum IS max_raw: the Viterbi path, the first maximum at every step."""
    v, back = model.start.tolist(), []
    for t in model.trans.tolist():
        nxt, arg = [], []
        for b in range(4):
            cand = [v[a] + t[4 * a + b] for a in range(4)]
            nxt.append(max(cand))
            arg.append(cand.index(max(cand)))
        v = nxt
        back.append(arg)
    b = v.index(max(v))
    path = [b]
    for arg in reversed(back):
        b = arg[b]
        path.append(b)
    return "".join("ACGT"[b] for b in reversed(path))


def same_planes(got, want):
    """Byte for byte: NaN where NaN, the same bits elsewhere, and the no-winner triple whole."""
    (gs, gp, gd), (ws, wp, wd) = got, want
    assert gs.dtype == np.float64 and gp.dtype == np.int32 and gd.dtype == np.int8
    assert gs.shape == ws.shape and np.array_equal(gp, wp) and np.array_equal(gd, wd)
    assert np.array_equal(np.isnan(gs), np.isnan(ws)) and np.array_equal(gs.view(np.int64)[~np.isnan(ws)], ws.view(np.int64)[~np.isnan(ws)])
    assert np.all(gp[np.isnan(gs)] == -1) and np.all(gd[np.isnan(gs)] == 0)


def with_n(seq, *at):
    b = bytearray(seq.encode())
    for i in at:
        b[i] = ord("N")
    return b.decode()


def n_cases(width, rng):
    """Regions around one window of `width` columns with an N on its first base, on its last base, and on the base just outside either
    end (the window itself is then whole), each with room for exactly one or two windows."""
    core = random_dna(rng, width + 2)
    out = [with_n(core, 1), with_n(core, width), with_n(core, 0), with_n(core, width + 1), with_n(core, 0, width + 1)]
    out.append(with_n(core[:width], 0))                   # the only window holds it: no winner
    if width > 1:
        out.append(with_n(core[:width], width - 1))
    return out


def small_models():
    """Per width of SMALL_WIDTHS a plain model and one with forbidden transitions."""
    models = []
    for w in SMALL_WIDTHS:
        models.append(random_model(w, 1000 + w))
        models.append(random_model(w, 2000 + w, holes=1 if w < 31 else 3))
    return models


def small_regions(seed=20260101):
    """Lengths W - 1, W, W + 1 of every small width, 63 / 64 / 65 window starts of a few widths, N placements of every small width, an
    N at a 32-base word edge, a region whose every window holds an N, lower case and an IUPAC letter."""
    rng = np.random.default_rng(seed)
    lengths = sorted({max(w + d, 0) for w in SMALL_WIDTHS for d in (-1, 0, 1)} | {w - 1 + n for w in (1, 2, 33, 65) for n in (63, 64, 65)})
    seqs = [random_dna(rng, n) for n in lengths]
    for w in SMALL_WIDTHS:
        seqs += n_cases(w, rng)
    edge = random_dna(rng, 130)
    seqs += [with_n(edge, 31), with_n(edge, 32), with_n(edge, 63, 64), with_n(edge, 95)]
    seqs.append(with_n(random_dna(rng, 40), *range(0, 40, 2)))                  # every window of two or more columns holds an N
    marked = bytearray(random_dna(rng, 150).encode())
    marked[40:90] = bytes(marked[40:90]).lower()
    marked[120] = ord("R")
    seqs.append(marked.decode())
    seqs.append("")                                                                # an empty region
    return seqs


def tie_cases():
    """(model, regions): a repeat whose every copy scores alike -- the earliest position must win --, and a reverse-palindromic site
    whose two strands score alike under a strand-symmetric model -- '+' must win."""
    m = random_model(6, 77)
    unit = "ACGGTCATTGCA"
    pal_pwm = np.array([[2.0, 0.1, 0.1, 0.1, 0.1, 0.1], [0.1, 2.0, 0.1, 0.1, 0.1, 0.1], [0.1, 0.1, 0.1, 0.1, 2.0, 0.1], [0.1, 0.1, 0.1, 0.1, 0.1, 2.0]])
    pal_pwm[:, 2] = [0.1, 0.1, 2.0, 0.1]                 # ACG | CGT: the consensus ACGCGT is its own reverse complement
    pal_pwm[:, 3] = [0.1, 2.0, 0.1, 0.1]
    pal_pwm = 0.5 * (pal_pwm + pal_pwm[::-1, ::-1])      # strand-symmetric: M[b][c] == M[3 - b][W - 1 - c]
    pal = dimodel.DiModel.from_pwm(pal_pwm)
    return [m, pal], [unit * 9, "TTTT" + "ACGCGT" + "TTTTT" + "ACGCGT" + "TT", unit[3:] + unit * 3]


def planted_case(seed=7, n=300, length=120):
    """300 input regions with one site drawn evenly from TGACGTCA / TGAGCTCA, 300 control regions with one decoy drawn evenly from
    TGACCTCA / TGAGGTCA, in an i.i.d. uniform background; and the PWM of the true sites (log-odds of their base counts + 1 against
    a uniform background, five decimals)."""
    rng = np.random.default_rng(seed)
    sites, decoys = ("TGACGTCA", "TGAGCTCA"), ("TGACCTCA", "TGAGGTCA")

    def regions(words):
        out = []
        for i in range(n):
            bg, at = random_dna(rng, length), int(rng.integers(0, length - 8 + 1))
            out.append(bg[:at] + words[i % 2] + bg[at + 8:])
        return out
    inputs, controls = regions(sites), regions(decoys)
    counts = np.ones((4, 8))
    for w in sites:
        for c, ch in enumerate(w):
            counts[CODE[ch], c] += n // 2
    pwm = np.around(np.log(counts / counts.sum(axis=0) / 0.25), 5)
    return inputs, controls, pwm


PLANTED_CUTOFF = 0.95                                     # of the PWM's normalised score: TGA[CG][CG]TCA exactly


def pwm_max_raw(m):
    """The scan's max_raw of a PWM: the column maxima clamped at 0, added in column order."""
    out = 0.0
    for c in range(m.shape[1]):
        out += max(0.0, float(m[:, c].max()))
    return out


def planted_hits_host(pwm, seqs, cutoff=PLANTED_CUTOFF):
    """The PWM's hits on N-free regions by ms_scan's rule (score - cutoff >= -1e-10), as ms_result-ordered arrays for
    sitestack.site_base_counts_host: (motif_offsets, seq_idx, pos, strand)."""
    deg, max_raw = dimodel.DiModel.from_pwm(pwm), pwm_max_raw(pwm)
    seq_idx, pos, strand = [], [], []
    for r, s in enumerate(seqs):
        fwd, rev = dimodel.window_sums_host(deg, s)
        for p in range(len(fwd)):
            for k, raw in ((1, fwd[p]), (2, rev[p])):
                if raw / max_raw - cutoff >= -1e-10:
                    seq_idx.append(r), pos.append(p), strand.append(k)
    return np.array([0, len(pos)]), np.array(seq_idx), np.array(pos), np.array(strand)
