"""
Every device entry point against what recycled memory holds.

The library takes its working memory, its result blocks and its pinned host blocks from caches of recycled blocks, and a recycled block
still holds what the call before left in it.  Each call site clears some of its sub-arrays by hand and lets its kernels write the rest;
the other GPU tests cannot see a clear that went missing, because the block a test gets is either fresh (often zero) or dirtied by the
same data ("a second call returns the same bytes" sets the same bits of an atomicOr bitmap again).

Here ms_debug_alloc_fill decides what a block holds when it is handed out.  A *case* builds its inputs on the host, runs one family of
entry points to completion, returns every output as numpy arrays and closes its handles.  Each case runs four times -- fill off, then
0x00, 0xFF (all-ones bitmaps, -1 integers, NaN doubles) and 0xA5 (finite garbage doubles, huge negative integers) -- with a different
case between its runs and the scan's persistent scratch released in front of every filled run.  Two things are asserted:
  (a) the fill-off outputs equal the reference the family's own GPU test uses (the oracle, or the host restatement: imported, not
      restated here);
  (b) every filled run equals the fill-off run byte for byte -- shape, dtype and tobytes().
ms_affinity_expected_counts is held to its restatement with the slack of tests/test_gpu_expected_counts.py and to its own fill-off run
byte for byte.

Shapes: motifs of 1, 5, 16 and 33 columns, one with a NaN entry, one with every entry <= 0; 67 regions (no multiple of 64) of 0, 4, 63,
64, 65 and 130 bases, one of N only, one of 2 * best_segment_windows() + 17 bases (the dense walks make partials), the rest 20 .. 100;
a total that is no multiple of 32, so that the last word of every plane has bits past the last base.  Run with -m gpu.
"""
import ctypes
import os
import random

import numpy as np
import pytest

import fuzz_parity as fz
import result_cases
from counts_cases import expected_counts
from motifscan_amd import _lib, affinity, annotation, em, enrich, footprint, kmers, personal, regions, scoredist, shuffle, sitestack
from test_em_host import assert_within_slack
from test_pairs_host import np_cooccurrence, np_pair_spacing
from test_scorehist_host import oracle_per_strand

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0xA5)
N_REGIONS = 67


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X (there is no CPU fallback)")
    _lib.set_device(0)


def pack(raw, offsets):
    """(codes, nmask, blk2reg, blkinfo) of the host packer"""
    return _lib.host_pack(np.frombuffer(bytes(raw), dtype=np.uint8), np.asarray(offsets, dtype=np.int64))


# ------------------------------------------------------------------------------------------------------------------ the world --

class World:
    """The inputs the cases share (host only), and the oracle's scans of them (made once, never changed)."""

    def __init__(self, oracle):
        rng = np.random.default_rng(20261021)
        self.seg = _lib.best_segment_windows()

        def mat(width):
            return np.round(rng.normal(0.0, 1.2, size=(4, width)), 3)

        holed = mat(7)
        holed[2, 3] = np.nan
        self.mats = [mat(1), mat(5), mat(16), mat(33), holed, -np.abs(mat(6)) - 0.001]
        self.nan_motif, self.neg_motif = 4, 5
        self.widths = np.array([m.shape[1] for m in self.mats], dtype=np.int32)
        self.vals = np.concatenate([m.ravel() for m in self.mats])
        self.cutoffs = np.array([0.9, 0.7, 0.55, 0.45, 0.5, 0.5])

        def seq(length, p_n=0.02):
            s = rng.choice(list("ACGTN"), size=length, p=[(1 - p_n) / 4] * 4 + [p_n]) if length else []
            return "".join(s)

        lengths = [0, 4, 63, 64, 65, 130, 40, 2 * self.seg + 17] + [int(x) for x in rng.integers(20, 101, size=N_REGIONS - 8)]
        self.seqs = [seq(n) for n in lengths]
        self.seqs[6] = "N" * 40
        self.seqs[9] = self.seqs[9].lower()
        order = rng.permutation(N_REGIONS)                   # the special regions anywhere in the set
        self.seqs = [self.seqs[i] for i in order]
        if sum(map(len, self.seqs)) % 32 == 0:
            self.seqs[-1] += "A"
        self.lengths = np.array([len(s) for s in self.seqs], dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self.raw = "".join(self.seqs).encode()
        self.n_bases = len(self.raw)
        assert len(self.seqs) == N_REGIONS and N_REGIONS % 64 and self.n_bases % 32
        assert {0, 4, 63, 64, 65, 130, 2 * self.seg + 17} <= set(self.lengths.tolist())
        self.want = {s: oracle.scan_arrays(self.vals, self.widths, self.cutoffs, self.raw, self.offsets, s, 4) for s in (1, 3)}
        assert len(self.want[3]["pos"]) > 1000
        self.planes = pack(self.raw, self.offsets)          # (codes, nmask, blk2reg, blkinfo) of the host packer
        # a genome of three chromosomes that holds the regions back to back, with a few bases around them
        self.chroms = {"c0": seq(77), "c1": "".join(self.seqs), "c2": seq(501, 0.1)}
        self.track = rng.integers(-1000, 1000, size=self.n_bases).astype(np.int32)

    def case_dict(self, strand):
        """the oracle's hits in the form of tests/result_cases.py"""
        return {"widths": self.widths, "n_regions": N_REGIONS, **self.want[strand]}


@pytest.fixture(scope="module")
def world(oracle):
    return World(oracle)


def pwmset(w):
    return _lib.PwmSet(w.vals, w.widths, w.cutoffs)


def hits_of(res):
    h = res.hits()
    return {k: np.array(h[k]) for k in ("motif_offsets", "seq_idx", "pos", "score", "strand")}


def same_hits(got, want, what):
    for k in ("motif_offsets", "seq_idx", "pos", "score"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs from the oracle"
    assert np.array_equal(got["strand"].astype(np.int32), want["strand"].astype(np.int32)), f"{what}: strand differs from the oracle"


def planes_out(out, name, sq):
    """codes, mask and the words behind them: identical whatever the block held, the bits past the last base included"""
    codes, nmask = sq.packed_host()
    pad_c, pad_n = _lib.seqset_pad_words(sq)
    out[name + ".codes"], out[name + ".nmask"], out[name + ".pad_codes"], out[name + ".pad_nmask"] = codes, nmask, pad_c, pad_n


def check_planes(out, name, want_codes, want_nmask, n_bases):
    assert np.array_equal(out[name + ".codes"], want_codes) and np.array_equal(out[name + ".nmask"], want_nmask), f"{name}: planes differ from the host packer"
    assert not out[name + ".pad_codes"].any() and not out[name + ".pad_nmask"].any(), f"{name}: the pad words are not zero"
    assert fz.plane_invariants_broken(out[name + ".codes"], out[name + ".nmask"], n_bases) is None, name


# ------------------------------------------------------------------------------------------------------------------ the cases --
# case(world, oracle) -> (outputs: dict of numpy arrays, check: a function of the outputs that holds them against the reference)

def case_seqset_makers(w, oracle):
    """ms_seqset_create, _create_hostpacked, the upload-only form packed by a scan, _from_device + repack: one set, four ways"""
    import torch
    out = {}
    for name, make in (("create", lambda: _lib.SeqSet(w.raw, w.offsets)), ("hostpacked", lambda: _lib.SeqSet(w.raw, w.offsets, host_pack_threads=3)),
                       ("keep_ascii", lambda: _lib.SeqSet(w.raw, w.offsets, keep_ascii=True))):
        sq = make()
        try:
            if name == "keep_ascii":
                sq.repack()
            planes_out(out, name, sq)
            out[name + ".blk2reg"], out[name + ".blkinfo"] = _lib.seqset_planes(sq)[2:]
        finally:
            sq.close()
    pw, sq = pwmset(w), _lib.seqset_upload_only(w.seqs)
    try:
        res = _lib.scan(pw, sq, 3)
        try:
            out["upload_only.hits"] = hits_of(res)["pos"]
        finally:
            res.close()
        planes_out(out, "upload_only", sq)
    finally:
        sq.close()
        pw.close()
    t = torch.zeros(w.n_bases + 32, dtype=torch.uint8, device="cuda:0")
    t[5:5 + w.n_bases] = torch.from_numpy(np.frombuffer(w.raw, dtype=np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    sq = _lib.SeqSet.from_device(t.data_ptr() + 5, w.offsets)
    try:
        planes_out(out, "from_device", sq)
    finally:
        sq.close()

    def check(o):
        for name in ("create", "hostpacked", "keep_ascii", "upload_only", "from_device"):
            check_planes(o, name, w.planes[0], w.planes[1], w.n_bases)
        for name in ("create", "hostpacked", "keep_ascii"):
            assert np.array_equal(o[name + ".blk2reg"], w.planes[2]) and np.array_equal(o[name + ".blkinfo"], w.planes[3]), name
        assert np.array_equal(o["upload_only.hits"], w.want[3]["pos"])
    return out, check


def _region_list(w):
    """the world's regions as (chromosome 1, start, end) of World.chroms, in an order of its own"""
    idx = np.arange(N_REGIONS)[::-1].copy()
    return np.ones(N_REGIONS, dtype=np.int32), w.offsets[idx], w.offsets[idx + 1], idx


def case_genome_makers(w, oracle):
    """ms_genome_create, ms_genome_create_packed, ms_seqset_from_genome, ms_genome_apply_alleles: planes through ms_genome_packed_host"""
    out = {}
    names = list(w.chroms)
    goff = np.concatenate([[0], np.cumsum([len(w.chroms[n]) for n in names])]).astype(np.int64)
    graw = "".join(w.chroms.values()).encode()
    g = _lib.ResidentGenome(w.chroms)
    try:
        packed = g.packed()
        out["genome.codes"], out["genome.nmask"] = np.array(packed.codes), np.array(packed.nmask)
        out["genome.pad_codes"], out["genome.pad_nmask"] = _lib.seqset_pad_words(g)
        g2 = _lib.ResidentGenome.from_packed(packed)
        try:
            codes, nmask = np.zeros_like(out["genome.codes"]), np.zeros_like(out["genome.nmask"])
            _lib.check(_lib.lib().ms_genome_packed_host(g2.h, _lib.ptr(codes, ctypes.c_uint32), _lib.ptr(nmask, ctypes.c_uint32)))
            out["packed.codes"], out["packed.nmask"] = codes, nmask
            out["packed.pad_codes"], out["packed.pad_nmask"] = _lib.seqset_pad_words(g2)
            out["packed.blk2reg"], out["packed.blkinfo"] = _lib.seqset_planes(g2)[2:]
        finally:
            g2.close()
        ci, st, en, idx = _region_list(w)
        cut = g.extract(ci, st, en)
        try:
            planes_out(out, "extract", cut)
        finally:
            cut.close()
        # a personal genome: an SNV, a deletion and an insertion in each of two chromosomes
        var = [(0, 3, 1, "T"), (0, 40, 5, ""), (0, 70, 0, "ACGTN"), (1, 0, 1, "g"), (1, int(goff[2] - goff[1]) - 3, 3, "A"), (1, 500, 2, "TTTTTTT")]
        alt_g, lm = _lib.apply_alleles(g, [v[0] for v in var], [v[1] for v in var], [v[2] for v in var], [v[3] for v in var])
        try:
            p = alt_g.packed()
            out["personal.codes"], out["personal.nmask"] = np.array(p.codes), np.array(p.nmask)
            out["personal.pad_codes"], out["personal.pad_nmask"] = _lib.seqset_pad_words(alt_g)
            out["personal.sizes"] = np.array(lm.alt_sizes)
            out["personal.status"] = np.array(lm.status)
            for c, name in enumerate(names[:2]):             # ms_liftmap_lift, every position of both chromosomes, both ways
                qa = np.arange(len(w.chroms[name]) + 1, dtype=np.int64)
                out[f"lift.to_alt{c}.pos"], out[f"lift.to_alt{c}.inside"] = lm.to_alt(np.full(qa.size, c, dtype=np.int32), qa)
                qr = np.arange(int(lm.alt_sizes[c]) + 1, dtype=np.int64)
                out[f"lift.to_ref{c}.pos"], out[f"lift.to_ref{c}.inside"] = lm.to_ref(np.full(qr.size, c, dtype=np.int32), qr)
        finally:
            lm.close()
            alt_g.close()
    finally:
        g.close()

    def check(o):
        want = pack(graw, goff)
        for name in ("genome", "packed"):
            check_planes(o, name, want[0], want[1], len(graw))
        assert np.array_equal(o["packed.blk2reg"], want[2]) and np.array_equal(o["packed.blkinfo"], want[3])
        ci, st, en, idx = _region_list(w)
        cut_raw = "".join(w.seqs[i] for i in idx).encode()
        cut_off = np.concatenate([[0], np.cumsum(w.lengths[idx])]).astype(np.int64)
        cw = pack(cut_raw, cut_off)
        check_planes(o, "extract", cw[0], cw[1], len(cut_raw))
        host = personal.apply_alleles_host([w.chroms[n] for n in names], [v[0] for v in var], [v[1] for v in var],
                                           [w.chroms[names[v[0]]][v[1]:v[1] + v[2]] for v in var], [v[3] for v in var])
        araw = b"".join(host["seqs"])
        aoff = np.concatenate([[0], np.cumsum(host["sizes"])]).astype(np.int64)
        aw = pack(araw, aoff)
        check_planes(o, "personal", aw[0], aw[1], len(araw))
        assert np.array_equal(o["personal.sizes"], host["sizes"]) and np.array_equal(o["personal.status"], host["status"])
        assert (host["status"] == 1).all()
        for c in range(2):
            for way in ("to_alt", "to_ref"):
                pos, inside = host[way][c]
                assert np.array_equal(o[f"lift.{way}{c}.pos"], pos) and np.array_equal(o[f"lift.{way}{c}.inside"], inside), (way, c)
    return out, check


def case_shuffle(w, oracle):
    """ms_seqset_shuffle, mono and dinuc: the new set's planes, pads and strings"""
    out = {}
    sq = _lib.SeqSet(w.raw, w.offsets)
    try:
        for kind in ("mono", "dinuc"):
            sh = sq.shuffled(kind, 77, 5)
            try:
                planes_out(out, kind, sh)
                out[kind + ".blk2reg"], out[kind + ".blkinfo"] = _lib.seqset_planes(sh)[2:]
            finally:
                sh.close()
    finally:
        sq.close()

    def check(o):
        for kind in ("mono", "dinuc"):
            seqs = shuffle.shuffle_host(w.seqs, kind, 77, 5)
            want = pack("".join(seqs).encode(), w.offsets)
            check_planes(o, kind, want[0], want[1], w.n_bases)
            assert np.array_equal(o[kind + ".blk2reg"], want[2]) and np.array_equal(o[kind + ".blkinfo"], want[3])
    return out, check


def case_scan(w, oracle):
    """ms_scan four ways (strand 1 and 3, pre-filter and all-fp64, counts only), and on the strand-3 result the compact forms, the site
    tables and ms_result_dedup"""
    out = {}
    pw, sq = pwmset(w), _lib.SeqSet(w.raw, w.offsets)
    try:
        for name, strand, flags in (("plus", 1, 0), ("both", 3, 0), ("exact", 3, _lib.MS_SCAN_EXACT_ONLY), ("counts", 3, _lib.MS_SCAN_COUNTS_ONLY)):
            res = _lib.scan(pw, sq, strand, flags)
            try:
                out[name + ".motif_offsets"], out[name + ".region_counts"] = np.array(res.motif_offsets), res.region_counts()
                if name == "counts":
                    continue
                for k, v in hits_of(res).items():
                    out[f"{name}.{k}"] = v
                if name == "both":
                    out["both.pageable.pos"] = res.hits_pageable()["pos"]
                    out["both.coord16"], out["both.score16"], _ = res.packed_words(16)
                    out["both.coord12"], out["both.score12"], shift = res.packed_words(12)
                    out["both.shift12"] = np.array([shift])
                    out["both.n_sites"], out["both.max_score"] = res.site_tables(N_REGIONS)
                    res.dedup(pw)
                    for k, v in hits_of(res).items():
                        out[f"dedup.{k}"] = v
                    out["dedup.region_counts"] = res.region_counts()
                    out["dedup.n_sites"], out["dedup.max_score"] = res.site_tables(N_REGIONS)
            finally:
                res.close()
    finally:
        sq.close()
        pw.close()

    def check(o):
        P = len(w.mats)
        for name, strand in (("plus", 1), ("both", 3), ("exact", 3)):
            same_hits({k: o[f"{name}.{k}"] for k in ("motif_offsets", "seq_idx", "pos", "score", "strand")}, w.want[strand], name)
        for name, strand in (("plus", 1), ("both", 3), ("exact", 3), ("counts", 3)):
            n, off, regions = expected_counts(w.want[strand], P)
            assert np.array_equal(o[name + ".motif_offsets"], off) and np.array_equal(o[name + ".region_counts"], regions), name
        case = w.case_dict(3)
        assert np.array_equal(o["both.pageable.pos"], case["pos"])
        assert np.array_equal(o["both.coord16"], result_cases.encode16(case)) and o["both.score16"].tobytes() == case["score"].tobytes()
        shift = result_cases.twelve_shift(N_REGIONS)
        assert int(o["both.shift12"][0]) == shift and np.array_equal(o["both.coord12"], result_cases.encode12(case, shift))
        assert o["both.score12"].tobytes() == case["score"].tobytes()
        n_sites, max_score = result_cases.site_tables_expected(case)
        assert np.array_equal(o["both.n_sites"], n_sites) and np.array_equal(o["both.max_score"], max_score, equal_nan=True)
        keep = result_cases.literal_keep(case)
        assert 0 < keep.sum() < len(keep)
        same_hits({k: o[f"dedup.{k}"] for k in ("motif_offsets", "seq_idx", "pos", "score", "strand")}, result_cases.filtered(case, keep), "dedup")
        assert np.array_equal(o["dedup.region_counts"], expected_counts(case, P)[2])
        n_sites, max_score = result_cases.site_tables_expected(case, keep)
        assert np.array_equal(o["dedup.n_sites"], n_sites) and np.array_equal(o["dedup.max_score"], max_score, equal_nan=True)
    return out, check


_BUCKETED = {}


def case_scan_bucketed(w, oracle):
    """a predicted-size scan whose hit list is written in buckets (the second scan of a set dense enough, forced as
    tests/test_gpu_bucketed_order.py forces it): hits, offsets, region counts"""
    from test_gpu_bucketed_order import N_MOTIFS, _mixed_regions
    from motifscan_amd import synth
    if not _BUCKETED:
        motifs = synth.load_motif_set(N_MOTIFS, p_value="1e-3")
        raw, offsets = _mixed_regions()
        _BUCKETED.update(motifs=motifs, raw=raw, offsets=offsets, want=oracle.scan_arrays(*motifs, raw, offsets, 3, 8))
    motifs, raw, offsets = _BUCKETED["motifs"], _BUCKETED["raw"], _BUCKETED["offsets"]
    env = {"MS_MEASURE": "1", "MS_RESCORE_SORTED_MIN": "0", "MS_SORT_LOW_BITS": "8", "MS_ORDER_BUCKETS": "1"}
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    out = {}
    try:
        pw, sq = _lib.PwmSet(*motifs), _lib.SeqSet(raw, offsets)
        try:
            for i in range(2):
                res = _lib.scan(pw, sq, 3)
                try:
                    for k, v in hits_of(res).items():
                        out[f"scan{i}.{k}"] = v
                    out[f"scan{i}.region_counts"] = res.region_counts()
                    st = res.stats()
                    out[f"scan{i}.form"] = np.array([st["order_bucketed"], st["n_passes"]])
                finally:
                    res.close()
        finally:
            sq.close()
            pw.close()
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def check(o):
        want = _BUCKETED["want"]
        for i in range(2):
            same_hits({k: o[f"scan{i}.{k}"] for k in ("motif_offsets", "seq_idx", "pos", "score", "strand")}, want, f"scan {i}")
            assert np.array_equal(o[f"scan{i}.region_counts"], expected_counts(want, len(motifs[1]))[2])
        assert o["scan0.form"].tolist() == [0, 1] and o["scan1.form"].tolist() == [1, 1], "the second scan was not bucketed"
    return out, check


def case_sweep_once_stream(w, oracle):
    """ms_scan_sweep, ms_scan_regions_once and one ms_stream with submit, submit_counts_only, submit_span and submit_regions (the pinned
    blocks, the queued scans)"""
    out = {}
    pw, g = pwmset(w), _lib.ResidentGenome(w.chroms)
    L1 = len(w.chroms["c1"])
    window, stride = 50, 37
    try:
        res = _lib.scan_sweep(pw, g, "c1", 3, L1 - 1, window, stride, 3)
        try:
            for k, v in hits_of(res).items():
                out[f"sweep.{k}"] = v
            out["sweep.region_counts"] = res.region_counts()
        finally:
            res.close()
        ci, st, en, idx = _region_list(w)
        res = _lib.scan_regions_once(pw, g, ci, st, en, 3)
        try:
            for k, v in hits_of(res).items():
                out[f"once.{k}"] = v
            out["once.region_counts"] = res.region_counts()
        finally:
            res.close()
        stream = _lib.Stream(pw, 3, _lib.MS_STREAM_PACKED12, depth=2)
        try:
            bases = np.frombuffer(w.raw, dtype=np.uint8).copy()
            span = np.frombuffer(w.chroms["c1"][3:L1 - 1].encode(), dtype=np.uint8).copy()
            stream.submit(bases, w.offsets)
            stream.submit(bases, w.offsets, counts_only=True)
            names = ["submit", "counts_only", "span", "regions"]
            got = [stream.next(), stream.next()]
            stream.submit_span(span, window, stride)
            stream.submit_regions(g, ci, st, en)
            got += [stream.next(), stream.next()]
            for name, res in zip(names, got):
                try:
                    out[f"stream.{name}.motif_offsets"], out[f"stream.{name}.region_counts"] = np.array(res.motif_offsets), res.region_counts()
                    if name != "counts_only":
                        h = res.hits(packed=True)
                        for k in ("seq_idx", "pos", "score", "strand"):
                            out[f"stream.{name}.{k}"] = np.array(h[k])
                finally:
                    res.close()
        finally:
            stream.close()
    finally:
        g.close()
        pw.close()

    def check(o):
        P = len(w.mats)
        chrom = w.chroms["c1"]
        n_win = (L1 - 1 - 3 - window) // stride + 1
        wins = [chrom[3 + k * stride:3 + k * stride + window] for k in range(n_win)]
        want_sweep = oracle.scan_arrays(w.vals, w.widths, w.cutoffs, "".join(wins).encode(), np.arange(n_win + 1, dtype=np.int64) * window, 3, 4)
        ci, st, en, idx = _region_list(w)
        want_once = oracle.scan_arrays(w.vals, w.widths, w.cutoffs, "".join(w.seqs[i] for i in idx).encode(),
                                       np.concatenate([[0], np.cumsum(w.lengths[idx])]).astype(np.int64), 3, 4)
        for name, want in (("sweep", want_sweep), ("once", want_once), ("stream.submit", w.want[3]), ("stream.span", want_sweep), ("stream.regions", want_once)):
            same_hits({k: o[f"{name}.{k}"] for k in ("motif_offsets", "seq_idx", "pos", "score", "strand")}, want, name)
            assert np.array_equal(o[name + ".region_counts"], expected_counts(want, P)[2]), name
        n, off, regions = expected_counts(w.want[3], P)
        assert np.array_equal(o["stream.counts_only.motif_offsets"], off) and np.array_equal(o["stream.counts_only.region_counts"], regions)
    return out, check


def case_variants(w, oracle):
    """ms_scan_variants, ms_scan_alleles and ms_scan_alleles_best on fuzz_parity's seeded cases (chunks of seven variants)"""
    from test_gpu_allelebest import expected_best, make_variants
    out = {}
    vc, ac = fz.make_variants_case(1), fz.make_alleles_case(10)
    prev = _lib.varscan_chunk(7)
    try:
        g, pw = _lib.ResidentGenome({f"c{i}": c for i, c in enumerate(vc["chroms"])}), _lib.PwmSet.from_matrices(vc["mats"], vc["cutoffs"])
        try:
            res = _lib.scan_variants(pw, g, vc["chrom_idx"], vc["pos"], vc["alt"], vc["strand"])
            try:
                for k, v in res.sites().items():
                    out["snv." + k] = np.array(v)
                out["snv.gained"], out["snv.lost"] = res.motif_counts()
                out["snv.ref_codes"] = res.ref_codes()
            finally:
                res.close()
        finally:
            pw.close()
            g.close()
        g, pw = _lib.ResidentGenome({f"c{i}": c for i, c in enumerate(ac["chroms"])}), _lib.PwmSet.from_matrices(ac["mats"], ac["cutoffs"])
        try:
            res = _lib.scan_alleles(pw, g, ac["chrom_idx"], ac["pos"], ac["ref_len"], ac["alts"], refs=ac["refs"], strand_mask=ac["strand"])
            try:
                for k, v in res.sites().items():
                    out["allele." + k] = np.array(v)
                out["allele.gained"], out["allele.lost"] = res.motif_counts()
                out["allele.ref_mismatch"] = res.ref_mismatch()
            finally:
                res.close()
            res = _lib.scan_alleles_best(pw, g, ac["chrom_idx"], ac["pos"], ac["ref_len"], ac["alts"], refs=ac["refs"], strand_mask=ac["strand"])
            try:
                for k, v in res.sites().items():
                    out["best." + k] = v
                out["best.ref_mismatch"] = res.ref_mismatch()
            finally:
                res.close()
        finally:
            pw.close()
            g.close()
    finally:
        _lib.varscan_chunk(prev)

    def check(o):
        want, _ = fz.expected_variants(oracle, vc)
        for k in ("motif_offsets", "variant", "start", "strand", "state", "gained", "lost", "ref_codes"):
            assert np.array_equal(o["snv." + k], want[k]), f"variants: {k}"
        assert fz.same_bits(o["snv.score_ref"], want["score_ref"]) and fz.same_bits(o["snv.score_alt"], want["score_alt"])
        want, _ = fz.expected_alleles(oracle, ac)
        for k in ("motif_offsets", "variant", "allele", "start", "strand", "gained", "lost", "ref_mismatch"):
            assert np.array_equal(o["allele." + k], want[k]), f"alleles: {k}"
        assert fz.same_bits(o["allele.score"], want["score"])
        var = make_variants([(int(c), int(x), int(r), a.encode()) for c, x, r, a in zip(ac["chrom_idx"], ac["pos"], ac["ref_len"], ac["alts"])])
        best = expected_best(oracle, {f"c{i}": c.encode() for i, c in enumerate(ac["chroms"])}, ac["mats"], var, ac["strand"])
        for k in _lib.AlleleBest.FIELDS:
            g_, w_ = o["best." + k], best[k]
            if k.startswith("score"):
                nan = np.isnan(w_)
                assert np.array_equal(np.isnan(g_), nan) and np.array_equal(g_.view(np.int64)[~nan], w_.view(np.int64)[~nan]), f"allele-best: {k}"
            else:
                assert np.array_equal(g_, w_), f"allele-best: {k}"
        assert np.array_equal(o["best.ref_mismatch"], want["ref_mismatch"])
    return out, check


def case_best(w, oracle):
    """ms_scan_best -> ms_best_rank_sum (the segmented sort form) and ms_best_count_passing"""
    out = {}
    pw, sq = pwmset(w), _lib.SeqSet(w.raw, w.offsets)
    sel_a, sel_b = np.arange(N_REGIONS) % 3 != 0, np.arange(N_REGIONS) % 3 == 0
    cut = np.tile(np.array([0.3, 0.5, 0.7]), (len(w.mats), 1))
    try:
        res = _lib.scan_best(pw, sq, 3)
        try:
            out["score"], out["pos"], out["strand"] = res.sites()
            u2, ties, na, nb = res.rank_sum(res, sel_a, sel_b)
            out["u2"], out["ties"], out["n"] = np.array(u2), np.array([[t & (2 ** 64 - 1), t >> 64] for t in ties], dtype=np.uint64), np.array([na, nb])
            out["passing"] = res.count_passing(cut, sel_a)
        finally:
            res.close()
    finally:
        sq.close()
        pw.close()

    def check(o):
        assert N_REGIONS <= _lib.ranksum_dims()["segmented_max"]
        walked = [m for m in range(len(w.mats)) if m not in (w.nan_motif, w.neg_motif)]      # (the other two are skipped: the documented fill)
        want = fz.oracle_best(oracle, [w.mats[m] for m in walked], w.seqs, 3)
        bad = fz.same_best((o["score"][walked], o["pos"][walked], o["strand"][walked]), want)
        assert bad is None, bad
        skipped = [w.nan_motif, w.neg_motif]
        assert np.isnan(o["score"][skipped]).all() and (o["pos"][skipped] == -1).all() and (o["strand"][skipped] == 0).all()
        rs = enrich.rank_sum_host(o["score"][:, sel_a], o["score"][:, sel_b])
        assert np.array_equal(o["u2"], rs.u2) and [int(lo) | (int(hi) << 64) for lo, hi in o["ties"].tolist()] == rs.ties
        assert o["n"].tolist() == [int(sel_a.sum()), int(sel_b.sum())]
        assert np.array_equal(o["passing"], enrich.count_passing_host(o["score"][:, sel_a], cut))
    return out, check


N_BINS = 16


def case_affinity(w, oracle):
    """ms_scan_affinity -> ms_affinity_rank_sum and ms_affinity_expected_counts (two blocks per tile: the grid-stride loop), and
    ms_scan_score_histogram"""
    out = {}
    pw, sq = pwmset(w), _lib.SeqSet(w.raw, w.offsets)
    sel_a, sel_b = np.arange(N_REGIONS) % 2 == 0, np.arange(N_REGIONS) % 2 == 1
    try:
        res = _lib.scan_affinity(pw, sq, 3, 1.0, -1)
        try:
            out["peak"], out["sum"], out["n_terms"], out["log_mean"] = res.cells()
            u2, ties, na, nb = res.rank_sum(res, sel_a, sel_b)
            out["u2"], out["ties"] = np.array(u2), np.array([[t & (2 ** 64 - 1), t >> 64] for t in ties], dtype=np.uint64)
            with _lib.expected_grid_cap(2):
                out["exp.counts"], out["exp.total"], out["exp.n_regions"] = res.expected_counts(pw, sq, 0.0)
        finally:
            res.close()
        out["hist"] = _lib.score_histogram(pw, sq, 3, -2.0, 1.5, N_BINS)
    finally:
        sq.close()
        pw.close()

    def check(o):
        host = affinity.affinity_host(w.mats, w.seqs, 3, 1.0, -1)
        assert np.array_equal(o["n_terms"], host.n_terms)
        both = ~np.isnan(host.peak)
        assert np.array_equal(np.isnan(o["peak"]), ~both) and o["peak"][both].tobytes() == host.peak[both].tobytes()
        assert (o["n_terms"][w.nan_motif] == 0).all() and np.isnan(o["log_mean"][w.nan_motif]).all()
        rs = enrich.rank_sum_host(o["log_mean"][:, sel_a], o["log_mean"][:, sel_b])
        assert np.array_equal(o["u2"], rs.u2) and [int(lo) | (int(hi) << 64) for lo, hi in o["ties"].tolist()] == rs.ties
        planes = (o["peak"], o["sum"], o["log_mean"], o["n_terms"])
        want, slack = em.expected_counts_host(w.mats, w.seqs, 3, 1.0, -1, 0.0, planes=planes)
        got = em.ExpectedCounts(o["exp.counts"], o["exp.total"], o["exp.n_regions"], [int(x) for x in w.widths])
        assert_within_slack(got, want, slack)
        assert got.counts.any()
        scorable = [m for m in range(len(w.mats)) if m not in (w.nan_motif, w.neg_motif)]
        want_h = oracle_per_strand(oracle, [w.mats[m] for m in scorable], w.seqs, 3, -2.0, 1.5, N_BINS)
        assert np.array_equal(o["hist"][scorable], want_h) and not o["hist"][[w.nan_motif, w.neg_motif]].any()
        assert np.array_equal(o["hist"], scoredist.restate_histogram(w.mats, w.seqs, 3, -2.0, 1.5, N_BINS))
    return out, check


def case_result_reductions(w, oracle):
    """on a result made with ms_result_from_hits of the oracle's sites: co-occurrence, pair spacing with an LDS histogram and with a
    global-memory one, site base counts (with dinucleotides) and the site signal over an ms_track"""
    out = {}
    c = w.case_dict(3)
    res = _lib.result_from_hits(len(w.mats), N_REGIONS, c["motif_offsets"], c["seq_idx"], c["pos"], c["score"], c["strand"])
    pw, sq, tr = pwmset(w), _lib.SeqSet(w.raw, w.offsets), _lib.Track(w.track, w.offsets)
    far = _lib.pair_lds_bins() // 2 + 1                     # 2 * far + 1 bins: the first histogram that does not fit LDS
    try:
        out["region_counts"] = res.region_counts()
        out["cooc"] = res.cooccurrence()
        out["cooc.rows"] = res.cooccurrence(1, 4)
        out["near.counts"], out["near.n_pairs"] = res.pair_spacing(pw, 1, 20)
        out["far.counts"], out["far.n_pairs"] = res.pair_spacing(pw, 2, far, 0, 3)
        out["stack.counts"], out["stack.dinuc"], out["stack.n_sites"] = res.site_base_counts(pw, sq, 3, dinuc=True)
        out["sig.sum"], out["sig.cover"], out["sig.n_sites"], out["sig.per_site"] = res.site_signal(pw, tr, 4, per_site=True)
        out["track"] = tr.values()
    finally:
        tr.close()
        sq.close()
        pw.close()
        res.close()

    def check(o):
        P = len(w.mats)
        off, seq_idx, pos, strand = c["motif_offsets"], c["seq_idx"], c["pos"], c["strand"]
        assert np.array_equal(o["region_counts"], expected_counts(c, P)[2])
        want = np_cooccurrence(off, seq_idx, P, N_REGIONS)
        assert np.array_equal(o["cooc"], want) and np.array_equal(o["cooc.rows"], want[1:4]) and want.any()
        counts, n_pairs = np_pair_spacing(off, seq_idx, pos, strand, w.widths, 1, 20)
        assert np.array_equal(o["near.counts"], counts) and np.array_equal(o["near.n_pairs"], n_pairs) and counts.any()
        assert 2 * far + 1 > _lib.pair_lds_bins() >= 41
        counts, n_pairs = np_pair_spacing(off, seq_idx, pos, strand, w.widths, 2, far)
        assert np.array_equal(o["far.counts"], counts[:3]) and np.array_equal(o["far.n_pairs"], n_pairs[:3]) and counts[:3].any()
        st = sitestack.site_base_counts_host(off, seq_idx, pos, strand, w.widths, w.seqs, 3, dinuc=True)
        assert np.array_equal(o["stack.counts"], st.counts) and np.array_equal(o["stack.dinuc"], st.dinuc) and np.array_equal(o["stack.n_sites"], st.n_sites)
        sg = footprint.site_signal_host(off, seq_idx, pos, strand, w.widths, w.track, w.offsets, 4)
        for k, got in (("sum", o["sig.sum"]), ("cover", o["sig.cover"]), ("n_sites", o["sig.n_sites"]), ("per_site", o["sig.per_site"])):
            assert np.array_equal(got, getattr(sg, k)), f"site signal: {k}"
        assert np.array_equal(o["track"], w.track)
    return out, check


def case_plot(w, oracle):
    """ms_result_site_histogram (LDS and global bins) and ms_result_rank_profile (raw and smoothed) on fuzz_parity's plot cases"""
    dims = _lib.plot_dims()
    cases = [fz.make_plot_case(seed, dims) for seed in (4, 9)]
    wide = dict(cases[0], extend=5 * dims["hist_lds_bins"] + 20)          # more bins than the LDS histogram holds
    out = {}
    for i, c in enumerate(cases + [wide]):
        n = int(c["motif_offsets"][-1])
        res = _lib.result_from_hits(c["P"], c["R"], c["motif_offsets"], c["region"], c["pos"], np.zeros(n), np.ones(n, dtype=np.int8))
        pw = _lib.PwmSet.from_matrices([np.full((4, int(x)), 0.25) for x in c["widths"]])
        try:
            out[f"{i}.counts"], out[f"{i}.n_sites"] = res.site_histogram(pw, c["summit_rel"], c["extend"])
            out[f"{i}.raw"] = res.rank_profile(c["order"], c["ratio"], smoothed=False)
            out[f"{i}.smooth"] = res.rank_profile(c["order"], c["ratio"], fz.expected_plot(c)[0]["smooth_k"])
        finally:
            pw.close()
            res.close()

    def check(o):
        assert fz.plot_n_bins(wide["extend"]) > dims["hist_lds_bins"] >= fz.plot_n_bins(cases[0]["extend"])
        for i, c in enumerate(cases + [wide]):
            want, _ = fz.expected_plot(c)
            assert np.array_equal(o[f"{i}.counts"], want["counts"]) and np.array_equal(o[f"{i}.n_sites"], want["n_sites"]), i
            assert fz.same_bits(o[f"{i}.raw"], want["raw"]), i
            for m in range(c["P"]):
                assert fz.plot_smoothed_differs(o[f"{i}.smooth"][m], want["raw"][m], want["smooth_k"]) is None, (i, m)
    return out, check


def case_kmers(w, oracle):
    """ms_seqset_kmer_counts at k = lds_k and lds_k + 1, with a sequence on either side of sort_windows and one bitmap per batch, and
    ms_genome_kmer_counts"""
    dims = _lib.kmer_dims()
    rng = np.random.default_rng(11)
    k_lo, k_hi, sw = dims["lds_k"], dims["lds_k"] + 1, dims["sort_windows"]
    long_a = "".join(rng.choice(list("ACGT"), size=sw + k_hi))              # more than sort_windows windows at either k: a bitmap
    long_b = "".join(rng.choice(list("ACGTN"), size=sw + k_hi + 40, p=[.24, .24, .24, .24, .04]))
    short = "".join(rng.choice(list("ACGT"), size=sw + k_lo - 1))           # exactly sort_windows windows at k_lo: sorted in LDS
    seqs = w.seqs[:20] + [long_a, short, long_b]
    out = {}
    sq, g = _lib.SeqSet.from_strings(seqs), _lib.ResidentGenome(w.chroms)
    prev = _lib.kmer_bitmap_budget(1)                                       # one bitmap per batch
    try:
        for k, canonical in ((k_lo, False), (k_hi, True)):
            r = sq.kmer_counts(k, canonical)
            out[f"k{k}.occ"], out[f"k{k}.nseq"], out[f"k{k}.totals"] = r.occ, r.nseq, np.array([r.n_seqs, r.n_windows, r.n_skipped, r.n_short])
        r = g.kmer_counts(3, True)
        out["genome.occ"], out["genome.nseq"] = r.occ, r.nseq
    finally:
        _lib.kmer_bitmap_budget(prev)
        g.close()
        sq.close()

    def check(o):
        for k, canonical in ((k_lo, False), (k_hi, True)):
            want = kmers.kmer_counts_host(seqs, k, canonical)
            assert np.array_equal(o[f"k{k}.occ"], want.occ) and np.array_equal(o[f"k{k}.nseq"], want.nseq), k
            assert o[f"k{k}.totals"].tolist() == [want.n_seqs, want.n_windows, want.n_skipped, want.n_short]
        want = kmers.kmer_counts_host(list(w.chroms.values()), 3, True)
        assert np.array_equal(o["genome.occ"], want.occ) and np.array_equal(o["genome.nseq"], want.nseq)
    return out, check


_GENOME = {}


def case_genome_jobs(w, oracle):
    """ms_genome_base_counts, ms_genome_window_filter, ms_score and ms_score_ranks on fuzz_parity's genome case, and
    ms_genes_nearest_tss / ms_genes_promoter_overlap on its annotation case"""
    if not _GENOME:
        gc = fz.make_genome_case(2, _lib.genome_dims())
        ann = fz.make_annot_case(2, _lib.genome_dims())
        _GENOME.update(gc=gc, ann=ann, want=fz.expected_genome(oracle, gc)[0], want_ann=fz.expected_annot(oracle, ann)[0])
    gc, ann, want, want_ann = _GENOME["gc"], _GENOME["ann"], _GENOME["want"], _GENOME["want_ann"]
    out = {}
    genome = _lib.ResidentGenome({f"c{i}": gc["bases"][gc["goff"][i]:gc["goff"][i + 1]] for i in range(len(gc["lens"]))})
    pw = _lib.PwmSet.from_matrices(gc["mats"])
    try:
        for i in (3, 6):                                                     # tile, clustered and not: LDS and global counters
            cl, a = gc["counts"][i]
            off = np.concatenate([[0], np.cumsum(cl)])
            g = _lib.ResidentGenome({f"c{j}": a[off[j]:off[j + 1]] for j in range(len(cl))})
            try:
                out[f"base_counts{i}"] = g.base_counts()
            finally:
                g.close()
        for k, call in enumerate(gc["calls"]):
            out[f"filter{k}"] = _lib.window_filter(genome, call["gstart"], call["length"], call["max_n"], want["exc_pos"], call["n_want"])
        sreg = np.array(want["score_regions"], dtype=np.int64)
        sq = genome.extract(sreg[:, 0], sreg[:, 1], sreg[:, 2])
        try:
            out["score"] = _lib.score(pw, sq, gc["strand"])
            prev = _lib.score_rank_budget(3 * len(sreg) + 1)                # batches of three motifs
            try:
                out["ranks"] = _lib.score_ranks(pw, sq, want["ranks"], gc["strand"])
            finally:
                _lib.score_rank_budget(prev)
        finally:
            sq.close()
    finally:
        pw.close()
        genome.close()
    genes = _lib.GeneTable(ann["off"], ann["tss"], ann["strand"])
    try:
        out["tss.dist"], out["tss.found"] = genes.nearest_tss(ann["near_chrom"], ann["near_start"], fz.ANNOT_CUTOFFS[0])
        for k, call in enumerate(ann["calls"][:2]):
            out[f"overlap{k}"] = genes.promoter_overlap(call["chrom"], call["start"], call["end"], call["upstream"], call["downstream"])
    finally:
        genes.close()

    def check(o):
        for i in (3, 6):
            assert np.array_equal(o[f"base_counts{i}"], want["counts"][i]), i
        for k, taken in enumerate(want["taken"]):
            assert np.array_equal(o[f"filter{k}"], taken), k
        assert fz.same_score_bits(o["score"], want["score"][gc["strand"]])
        keep = want["rank_compared"]
        assert fz.same_score_bits(o["ranks"][keep], want["rank_rows"][keep])
        wd, wf = want_ann["nearest"][fz.ANNOT_CUTOFFS[0]]
        assert np.array_equal(o["tss.dist"], wd) and np.array_equal(o["tss.found"], wf)
        for k in range(2):
            assert np.array_equal(o[f"overlap{k}"], want_ann["overlap"][k]), k
    return out, check


_CONTROL = {}


def case_control_regions(w, oracle):
    """the control-region generator with genes (regions.generate_control_regions: the replay on the host, ms_genes_nearest_tss at the
    reference's cutoff on the device, through a gene table made anew), and the set of its regions cut from a resident genome"""
    if not _CONTROL:
        d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_regions.npz"))
        _CONTROL.update({k: d[k] for k in d.files})
        chroms = [str(c) for c in _CONTROL["reg_chroms"]]
        rng = np.random.default_rng(5)
        _CONTROL["chroms"] = chroms
        _CONTROL["bases"] = {c: np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.choice(5, size=int(n), p=[.24, .24, .24, .24, .04])]
                             for c, n in zip(chroms, _CONTROL["chrom_size"])}
    g_ = _CONTROL
    chroms = g_["chroms"]
    regs = [regions.GenomicRegion(chroms[c], s_, e_) for c, s_, e_ in zip(g_["reg_chrom"].tolist(), g_["reg_start"].tolist(), g_["reg_end"].tolist())]
    sizes = {c: int(n) for c, n in zip(chroms, g_["chrom_size"])}
    genes = annotation.Genes.from_arrays([str(c) for c in g_["gene_chrom"]], g_["gene_tss"], g_["gene_strand"])
    state = random.getstate()
    out = {}
    try:
        got = regions.generate_control_regions(5, regs, sizes, genes=genes, random_seed=3)
    finally:
        random.setstate(state)
        genes.table().close()
    ci = np.array([chroms.index(got.chroms[c]) for c in got.chrom_idx], dtype=np.int32)
    out["chrom"], out["start"], out["end"] = ci, np.array(got.start), np.array(got.end)
    genome = _lib.ResidentGenome(g_["bases"])
    try:
        cut = genome.extract(ci, got.start, got.end)
        try:
            planes_out(out, "cut", cut)
        finally:
            cut.close()
    finally:
        genome.close()

    def check(o):
        assert np.array_equal(o["chrom"], g_["ctl_1_3_5_chrom"]) and np.array_equal(o["start"], g_["ctl_1_3_5_start"]) and np.array_equal(o["end"], g_["ctl_1_3_5_end"])
        raw = b"".join(g_["bases"][chroms[c]][a:b].tobytes() for c, a, b in zip(o["chrom"].tolist(), o["start"].tolist(), o["end"].tolist()))
        off = np.concatenate([[0], np.cumsum(o["end"] - o["start"])]).astype(np.int64)
        want = pack(raw, off)
        check_planes(o, "cut", want[0], want[1], len(raw))
    return out, check


CASES = {
    "control_regions": case_control_regions,
    "seqset_makers": case_seqset_makers,
    "genome_makers": case_genome_makers,
    "shuffle": case_shuffle,
    "scan": case_scan,
    "scan_bucketed": case_scan_bucketed,
    "sweep_once_stream": case_sweep_once_stream,
    "variants": case_variants,
    "best": case_best,
    "affinity": case_affinity,
    "result_reductions": case_result_reductions,
    "plot": case_plot,
    "kmers": case_kmers,
    "genome_jobs": case_genome_jobs,
}
# the case that runs between two runs of a case: other data through the same size classes (bitmaps, flags, planes, the scan's scratch)
BETWEEN = {name: ("result_reductions" if name in ("scan", "kmers", "plot") else "scan") for name in CASES}
BETWEEN["result_reductions"] = "kmers"


def flat(out):
    """the outputs as a flat dict of arrays"""
    res = {}
    for k, v in out.items():
        assert isinstance(v, np.ndarray), (k, type(v))
        res[k] = v
    return res


def assert_same_bytes(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k} has shape {a.shape} {a.dtype}, not {b.shape} {b.dtype}"
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero(np.ascontiguousarray(a).reshape(-1).view(np.uint8) != np.ascontiguousarray(b).reshape(-1).view(np.uint8))
            raise AssertionError(f"{what}: {k} differs from the run without a fill in {len(bad)} bytes, the first at byte {int(bad[0])}")


FAULTS = ("illegal memory access", "memory access fault", "unspecified launch failure", "launch failure", "hardware exception", "device-side assert",
          "hipErrorIllegalAddress", "hipErrorLaunchFailure")


def run(case, world, oracle):
    """One run of a case.  A device FAULT ends the session: a kernel that read an index out of an unwritten word has faulted, and
    nothing more may start on that device.  Any other error of the library fails the test that met it."""
    try:
        return case(world, oracle)
    except RuntimeError as e:
        if any(f in str(e) for f in FAULTS):
            pytest.exit(f"{case.__name__}: the device faulted ({e}); no further GPU test is started", returncode=3)
        raise


@pytest.mark.parametrize("name", sorted(CASES))
def test_outputs_do_not_depend_on_what_the_blocks_held(world, oracle, name):
    case, other = CASES[name], CASES[BETWEEN[name]]
    with _lib.alloc_fill(-1):
        off, check = run(case, world, oracle)
    off = flat(off)
    check(off)                                               # (a) the reference of the family's own test
    for fill in FILLS:
        run(other, world, oracle)                            # other data through the same blocks, no fill
        _lib.release_scratch()                               # the scan's persistent arrays come back through the filled allocator
        with _lib.alloc_fill(fill) as before:
            assert before == -1
            got, _ = run(case, world, oracle)
        assert_same_bytes(flat(got), off, f"{name} under fill 0x{fill:02X}")       # (b)


def test_live_handles_survive_later_fills(world, oracle):
    """a block that went back to the cache while a handle still points into it would be filled under that handle"""
    w = world
    pw, sq = pwmset(w), _lib.SeqSet(w.raw, w.offsets)
    res, best = _lib.scan(pw, sq, 3), _lib.scan_best(pw, sq, 3)
    try:
        def read():
            out = {"scan." + k: v for k, v in hits_of(res).items()}
            out["scan.pageable"] = res.hits_pageable()["score"]
            out["scan.region_counts"] = res.region_counts()
            out["best.score"], out["best.pos"], out["best.strand"] = best.sites()
            planes_out(out, "set", sq)
            out["set.blk2reg"], out["set.blkinfo"] = _lib.seqset_planes(sq)[2:]
            return out
        first = read()
        same_hits({k: first["scan." + k] for k in ("motif_offsets", "seq_idx", "pos", "score", "strand")}, w.want[3], "scan")
        with _lib.alloc_fill(0xFF):
            for name in ("result_reductions", "kmers", "shuffle"):
                run(CASES[name], w, oracle)
        res._hits = None                                     # read the device arrays again, not the copy the object keeps
        assert_same_bytes(read(), first, "the live handles after three cases under fill 0xFF")
    finally:
        best.close()
        res.close()
        sq.close()
        pw.close()


def device_words(address, n):
    """n 64-bit words of device memory at `address`, through torch (as tests/test_gpu_allelebest.py reads the library's device arrays)"""
    import torch
    from test_gpu_allelebest import _DevicePtr
    return torch.as_tensor(_DevicePtr(address, n, "<i8"), device="cuda:0").cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("fill", FILLS)
def test_the_hook_fills_and_the_makers_clear(world, fill):
    """under each fill byte: a word the library never writes holds the fill (the hook reaches memory); a set's blocks come fresh and then
    recycled, its pad words zero and its planes the host packer's both times; the pinned cache is hit; the hook round-trips"""
    w = world
    with _lib.alloc_fill(fill) as before:
        assert before == -1
        with _lib.alloc_fill(fill ^ 0x3C) as inner:
            assert inner == fill
        _lib.pool_trim()
        pin0 = _lib.host_pool_stats()
        for fresh in (True, False):                          # the set's blocks straight from the driver, then the same blocks recycled
            s0 = _lib.pool_stats()
            sq = _lib.SeqSet(w.raw, w.offsets)
            try:
                s1 = _lib.pool_stats()
                assert (s1["misses"] > s0["misses"], s1["hits"] > s0["hits"]) == (fresh, not fresh), (fresh, s0, s1)
                out = {}
                planes_out(out, "set", sq)
                check_planes(out, "set", w.planes[0], w.planes[1], w.n_bases)
            finally:
                sq.close()
            # ms_result_from_hits uploads P region counts into a slot of P + 1 words: the last one is never written (ALLOCATIONS.md)
            c = w.case_dict(3)
            res = _lib.result_from_hits(len(w.mats), N_REGIONS, c["motif_offsets"], c["seq_idx"], c["pos"], c["score"], c["strand"])
            try:
                words = device_words(res.region_counts_device_ptr(), len(w.mats) + 1)
                assert np.array_equal(words[:-1].astype(np.int64), expected_counts(c, len(w.mats))[2])
                assert int(words[-1]) == int.from_bytes(bytes([fill]) * 8, "little"), (fresh, hex(int(words[-1])))
            finally:
                res.close()
        assert _lib.host_pool_stats()["hits"] > pin0["hits"]      # the second set's offsets went through a recycled pinned block
    prev = ctypes.c_int32(7)
    for bad in (-2, 256, 1 << 20):
        assert _lib.lib().ms_debug_alloc_fill(bad, ctypes.byref(prev)) == _lib.MS_ERR_INVALID and prev.value == 7
    assert _lib.lib().ms_debug_alloc_fill(-1, ctypes.byref(prev)) == _lib.MS_OK and prev.value == -1
