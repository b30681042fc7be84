"""
order_finalize_kernel's staged window (ms_order.hip): a block owns the runs that start in its tile of the radix-ordered list and stages the
keys of `ext` more slots to close the tile's last run.  The host takes the window per scan from the expected run n / (P x 2^(gbits + 1 - L)):
960 + 64 slots up to one hit, 1024 + 256 above.  A run is left to order_overflow_kernel when it is longer than MS_ORDER_RUN_CAP, or when it
does not close inside its block's window -- which only a run longer than the extension can fail to do.

Every run here is built: poly-A stretches under the word AAAAAAAA give one hit per window start on the plus strand, TTTTTTTT the same hits on
the minus strand, and the rest of every region alternates A and C, where neither word and none of the G/C filler words can hit.  Regions are
500 bases (9 position bits), so at L = 16 a run is one motif's hits in a group of 64 regions, and at L = 8 one motif's hits in a 128-base
stretch of one region.  The filler words only raise the motif count, which is how a case picks its window.  Each case checks the run
lengths it means to have on the oracle's hits, compares hits, offsets and region counts with the oracle bit for bit, and compares
`order_overflow_runs` with a model of the rule above.

Measurement switches (honoured only with MS_MEASURE=1): MS_SORT_LOW_BITS forces L, MS_ORDER_RUN_CAP the cap.
"""
import numpy as np
import pytest

from motifscan_amd import _lib

pytestmark = pytest.mark.gpu

REGION = 500
STRETCH_AT = 130              # a stretch's hits start here: up to 100 of them stay inside the positions 128 ... 255
SHORT, LONG = (960, 64), (1024, 256)          # (tile, extension) of the two windows
SHORT_MEAN_RUN = 1.0


@pytest.fixture(scope="module", autouse=True)
def device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X (there is no CPU fallback)")
    _lib.set_device(0)


def _set_env(monkeypatch, low_bits, run_cap=None):
    monkeypatch.setenv("MS_MEASURE", "1")
    monkeypatch.setenv("MS_SORT_LOW_BITS", str(low_bits))
    if run_cap is None:
        monkeypatch.delenv("MS_ORDER_RUN_CAP", raising=False)
    else:
        monkeypatch.setenv("MS_ORDER_RUN_CAP", str(run_cap))


def _word_motif(word):
    m = np.full((4, len(word)), -3.0)
    for c, b in enumerate(word):
        m["ACGT".index(b), c] = 1.25
    return m


def _motifs(n_filler, minus=True):
    rng = np.random.default_rng(77)
    words = ["AAAAAAAA"] + (["TTTTTTTT"] if minus else []) + ["".join(rng.choice(list("GC"), size=8)) for _ in range(n_filler)]
    mats = [_word_motif(w) for w in words]
    return (np.concatenate([m.ravel() for m in mats]), np.full(len(words), 8, dtype=np.int32), np.full(len(words), 0.95))


def _region(c):
    """500 bases with exactly c windows of eight A, at the positions STRETCH_AT ... STRETCH_AT + c - 1; none: 120 bases (the oracle's time)"""
    assert 0 <= c <= 100
    if c == 0:
        return "AC" * 60
    head = "AC" * (STRETCH_AT // 2) + "A" * (c + 7)
    return head + ("CA" * REGION)[:REGION - len(head)]


def _regions(group_hits, n_groups, per_region=100):
    """group g (the regions 64 g ... 64 g + 63) holds group_hits[g] hits, per_region to a region from the group's first region on"""
    assert len(group_hits) <= n_groups
    seqs = []
    for g in range(n_groups):
        left = group_hits[g] if g < len(group_hits) else 0
        assert left <= 64 * per_region
        for _ in range(64):
            c = min(left, per_region)
            seqs.append(_region(c))
            left -= c
    assert seqs[-1] == _region(0)
    seqs[-1] = "AC" * (REGION // 2)                                # nine position bits whatever the groups hold
    raw = "".join(seqs).encode()
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return raw, offsets


def _bits(n):
    return max(1, int(n - 1).bit_length())


def _runs(want, P, R, low_bits):
    """lengths of the runs of equal key >> L in the final order, key = motif | region | position | strand bit, and the list's layout"""
    rbits, pbits = _bits(R), _bits(REGION)
    motif = np.repeat(np.arange(P, dtype=np.int64), np.diff(want["motif_offsets"]))
    key = (motif << (rbits + pbits + 1)) | (want["seq_idx"].astype(np.int64) << (pbits + 1)) | (want["pos"].astype(np.int64) << 1) \
        | (want["strand"].astype(np.int64) == 2)
    assert (np.diff(key) > 0).all()
    edges = np.flatnonzero(np.diff(key >> low_bits)) + 1
    starts = np.concatenate([[0], edges])
    return starts, np.diff(np.concatenate([starts, [len(key)]])), rbits + pbits


def _window(n, P, gbits, low_bits):
    """the window the host takes for a list of n hits; None within a factor of two of the rule's threshold (a predicted-size scan's n is a few
    per cent above the hits it finds)"""
    mean = n / P * 2.0 ** (low_bits - gbits - 1)
    if 0.5 * SHORT_MEAN_RUN < mean <= 2.0 * SHORT_MEAN_RUN:
        return None
    return SHORT if mean <= SHORT_MEAN_RUN else LONG


def _overflow_model(starts, lens, n, window, run_cap):
    tile, ext = window
    at = starts % tile
    open_end = (at + lens > tile + ext) | ((at + lens == tile + ext) & (starts + lens < n))
    return int((open_end | (lens > run_cap)).sum())


def _region_counts(want, P):
    off = want["motif_offsets"]
    return np.array([len(np.unique(want["seq_idx"][off[p]:off[p + 1]])) for p in range(P)], dtype=np.int64)


def _check(monkeypatch, motifs, raw, offsets, strand, want, low_bits, window, run_cap=None, what=""):
    P, R = len(motifs[1]), len(offsets) - 1
    starts, lens, gbits = _runs(want, P, R, low_bits)
    n = len(want["pos"])
    assert gbits <= int(offsets[-1]).bit_length() + 2              # the keys carry (region, position): the form this kernel serves
    assert _window(n, P, gbits, low_bits) == window, f"{what}: the case was built for another window"
    expect = _overflow_model(starts, lens, n, window, run_cap if run_cap is not None else 1 << 30)
    _set_env(monkeypatch, low_bits, run_cap)
    pw, sq = _lib.PwmSet(*motifs), _lib.SeqSet(raw, offsets)
    for i in range(2):                                             # the exactly-sized form, then the predicted one (padding keys behind the hits)
        res = _lib.scan(pw, sq, strand)
        got = res.hits()
        for k in ("motif_offsets", "seq_idx", "pos", "score"):
            assert np.array_equal(got[k], want[k]), f"{what}, scan {i}: {k} differs"
        assert np.array_equal(got["strand"].astype(np.int32), want["strand"].astype(np.int32)), f"{what}, scan {i}: strand differs"
        assert np.array_equal(np.asarray(res.region_counts(), dtype=np.int64), _region_counts(want, P)), f"{what}, scan {i}: region counts differ"
        st = res.stats()
        assert st["n_passes"] == 1 and st["order_bucketed"] == 0
        assert st["order_overflow_runs"] == expect, f"{what}, scan {i}: runs left to the overflow kernel"
        res.close()
    return expect


def _pad_to(hits, slot, most=60):
    """runs of at most `most` hits (shorter than either extension) until the next run starts at `slot`"""
    at = sum(hits)
    assert at <= slot
    while at < slot:
        hits.append(min(most, slot - at))
        at += hits[-1]


def _edge_layout(window, run_cap):
    """Group hit counts whose runs, at L = 16, meet every edge of `window` and of the cap: runs of ext - 1, ext, ext + 1 and cap - 1, cap,
    cap + 1 hits inside a tile; a run of ext hits from a tile's last slot (it closes on the window's last slot) and one of ext + 1 from
    there (it does not); a run that straddles a tile boundary and closes well inside the extension; a run as long as the tile."""
    tile, ext = window
    hits = []
    _pad_to(hits, 100)
    hits += [ext - 1, 7, ext, 9, ext + 1, 3, run_cap - 1, run_cap, run_cap + 1]
    assert sum(hits) <= tile - 1
    _pad_to(hits, tile - 1)
    hits.append(ext)                        # slots tile - 1 ... tile + ext - 2
    _pad_to(hits, 2 * tile - 1)
    hits.append(ext + 1)                    # slots 2 tile - 1 ... 2 tile + ext - 1: one past the window
    _pad_to(hits, 3 * tile - 20)
    hits.append(45)                         # straddles 3 tile
    _pad_to(hits, 4 * tile - 5)
    hits.append(tile)                       # starts in one tile, covers the next
    hits.append(11)
    return hits


N_GROUPS = 80          # 5120 regions, 2.56 Mbases: 13 region bits, 22 coordinate bits


@pytest.fixture(scope="module")
def edges(oracle):
    """per window: the motif set that selects it, the sequences, the oracle's hits for both strands"""
    out = {}
    for window, n_filler in ((SHORT, 400), (LONG, 2)):
        motifs = _motifs(n_filler)
        raw, offsets = _regions(_edge_layout(window, 40), N_GROUPS)
        out[window] = (motifs, raw, offsets, oracle.scan_arrays(*motifs, raw, offsets, 3, 8))
    return out


@pytest.mark.parametrize("run_cap", [None, 40])
@pytest.mark.parametrize("window", [SHORT, LONG])
def test_runs_at_the_edges_of_the_window_and_of_the_cap(edges, monkeypatch, window, run_cap):
    motifs, raw, offsets, want = edges[window]
    tile, ext = window
    P = len(motifs[1])
    starts, lens, _ = _runs(want, P, len(offsets) - 1, 16)
    half = len(lens) // 2                   # the plus-strand word's runs, then the same runs under the minus-strand word
    assert np.array_equal(lens[:half], lens[half:]) and set(want["strand"][:want["motif_offsets"][1]]) == {1}
    assert set(want["strand"][want["motif_offsets"][1]:]) == {2}
    for m in (ext - 1, ext, ext + 1, 39, 40, 41, tile):
        assert m in lens[:half]
    assert lens[:half][starts[:half] == tile - 1] == ext and lens[:half][starts[:half] == 2 * tile - 1] == ext + 1
    s45 = starts[:half][lens[:half] == 45]
    assert len(s45) == 1 and s45[0] < 3 * tile < s45[0] + 45
    n_over = _check(monkeypatch, motifs, raw, offsets, 3, want, 16, window, run_cap, f"window {window}, cap {run_cap}")
    assert n_over >= (2 if run_cap is None else 8)


@pytest.mark.parametrize("window", [SHORT, LONG])
def test_eight_low_bits(edges, monkeypatch, window):
    """The same sequences at L = 8: a run is a region's stretch, at most 100 hits.  Both motif sets give the short window there (no list of this
    size has a mean run above one at L = 8), under which the stretches of more than 64 hits that start late in a tile are left to the overflow kernel."""
    motifs, raw, offsets, want = edges[window]
    _, lens, _ = _runs(want, len(motifs[1]), len(offsets) - 1, 8)
    assert lens.max() == 100 and (window == LONG or {63, 64, 65} <= set(lens.tolist()))
    _check(monkeypatch, motifs, raw, offsets, 3, want, 8, SHORT, None, f"L = 8, motif set of window {window}")


@pytest.fixture(scope="module")
def lengths(oracle):
    """lists of exactly n hits in runs of at most 40 (L = 8: one stretch a region), one word on the plus strand"""
    out = {}
    for n in (1, 959, 960, 961, 1024, 1025, 1088, 1280, 1281):
        raw, offsets = _regions([n], 1, per_region=40)
        for n_filler in (0, 63):
            motifs = _motifs(n_filler, minus=False)
            out[n, n_filler] = (motifs, raw, offsets, oracle.scan_arrays(*motifs, raw, offsets, 1, 4))
    return out


@pytest.mark.parametrize("n_filler", [0, 63])
@pytest.mark.parametrize("n", [1, 959, 960, 961, 1024, 1025, 1088, 1280, 1281])
def test_list_lengths_around_the_tiles(lengths, monkeypatch, n, n_filler):
    """A list that ends on, one short of and one past a tile and a window of either kind.  One motif: mean run n / 256 at L = 8, the long window
    from 512 hits on; 64 motifs: the short one."""
    motifs, raw, offsets, want = lengths[n, n_filler]
    assert len(want["pos"]) == n
    P = len(motifs[1])
    window = LONG if (P == 1 and n > 512) else SHORT
    assert _check(monkeypatch, motifs, raw, offsets, 1, want, 8, window, None, f"{n} hits, {P} motifs") == 0
