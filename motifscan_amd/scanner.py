"""
motifscan_amd.scanner -- host-side mirror of the reference's `motifscan.scanner`
(/root/reference/motifscan/scanner.py) over the MI355X scan path.

Same public surface and behaviour:
    MotifSite(start, score, strand)                      scanner.py:16
    Scanner(genome, regions, window_size=0, strand='both', p_value='1e-4',
            remove_dup=True, n_threads=1)                scanner.py:44-69
        .sequences / .seq_starts / .seq_ends / .window_size / .extend / .strand /
        .p_value / .remove_dup / .n_threads
        .scan_motifs(pwms) -> nested list [n_pwms][n_regions] of MotifSite   scanner.py:89-132
    make_motif_sites(sites, seq_starts)                  scanner.py:135-153
    deduplicate_motif_sites(motif_sites, lengths)        scanner.py:171-193
plus, for inputs where n_pwms x n_regions Python lists are not an option:
    Scanner.scan_motifs_arrays(pwms) -> flat numpy arrays in the same order.
and the questions the reference cannot answer from its site lists:
    Scanner.best_sites(pwms) -> BestSiteArrays: the best-scoring window of every (motif, region), cutoff or not.
    Scanner.rank_sum(pwms, control) -> enrich.RankSum: cutoff-free enrichment of the best scores against a control scanner's.
    Scanner.count_regions_passing(pwms, cutoffs) -> the regions with >= 1 site at several cutoffs per motif, from one scan.
    Scanner.best_sites_bipartite(pwms, specs) -> bipartite.BipartiteSites: the best placement of two half-sites with a variable spacer.
    Scanner.rank_sum_bipartite(pwms, specs, control) -> enrich.RankSum: rank_sum over those best placements.
    Scanner.affinity(pwms) -> affinity.AffinityArrays: the likelihood ratio summed over ALL windows of every (motif, region).
    Scanner.affinity_rank_sum(pwms, control) -> enrich.RankSum: rank_sum with that sum in place of the best score.
    Scanner.expected_counts(pwms, gamma) -> em.ExpectedCounts: per motif column the A, C, G, T weight over ALL windows, each weighted by
                                            its posterior probability of being the site (the E-step of a motif refinement).
    Scanner.refine_motifs(pwms, ...) -> em.Refinement: expectation maximisation of the matrices over the regions, without a cutoff.
    Scanner.score_histogram(pwms, ...) -> scoredist.ScoreHistogram: the score distribution of all windows, per motif.
    Scanner.site_base_counts(pwms, ...) -> sitestack.SiteStack: the base counts per motif column over the sites found.
    Scanner.site_signal(pwms, track, ...) -> footprint.SiteSignal: a per-base track summed per motif column over the sites found.

`genome` is any object with `chrom_sizes[chrom]` and `fetch_sequence(chrom, start, end)`;
`regions` any objects with `.chrom .start .end .summit` -- i.e. the reference's own
`Genome` / `GenomicRegion` work unchanged.  `pwms` is any iterable of objects with
`.matrix` (4 x W), `.cutoffs[p_value]` and `.length`.
"""
import logging
import os

import numpy as np

from . import _lib
from .regions import RegionArray
from .sites import MotifSite, MotifSites, RegionSites  # noqa: F401  (MotifSite is part of this module's surface, scanner.py:16)

logger = logging.getLogger(__name__)

_STRAND_FLAG = {"+": 1, "-": 2, "both": 3}


class _Frozen(list):
    """The scanner's region lists: real lists to read (==, len, index, slices), but the regions are FROZEN after construction --
    the packed device copy made on the first scan is kept for the scanner's life, so an edit would be silently ignored by
    scan_motifs while scan_batches re-encodes the strings.  Every mutating method raises instead."""
    __slots__ = ()

    def _refuse(self, *a, **k):
        raise TypeError("a Scanner's regions are frozen after construction (its packed device copy is cached): build a new Scanner")

    __setitem__ = __delitem__ = __iadd__ = __imul__ = append = extend = insert = pop = remove = clear = sort = reverse = _refuse


class BestSiteArrays:
    """Scanner.best_sites: (n_pwms, n_regions) arrays -- score (float64, NaN where no window wins), start (int64, the window's start
    in genome coordinates, -1 where none) and strand (int8: 1 '+', 2 '-', 0 where none: the library's strand flags, as
    scan_motifs_arrays gives them)."""
    __slots__ = ("score", "start", "strand")

    def __init__(self, score, start, strand):
        self.score, self.start, self.strand = score, start, strand


def best_site_starts(pos, seq_starts):
    """Positions relative to the region start (P, R; -1 = none) -> genome coordinates, -1 kept.  Pure host code."""
    pos = np.asarray(pos)
    starts = np.asarray(seq_starts, dtype=np.int64).reshape(1, -1)
    if pos.ndim != 2 or pos.shape[1] != starts.shape[1]:
        raise ValueError("pos must be (P, R) with one column per region")
    return np.where(pos >= 0, pos.astype(np.int64) + starts, np.int64(-1))


class Scanner:
    def __init__(self, genome, regions, window_size=0, strand="both", p_value="1e-4", remove_dup=True,
                 n_threads=1):
        self.window_size = window_size if window_size > 0 else 0
        self.extend = window_size // 2
        if strand not in _STRAND_FLAG:
            raise ValueError(f"invalid strand option: {strand!r}")
        self.strand = strand
        self.p_value = p_value
        self.remove_dup = remove_dup
        # kept for interface parity; the GPU path has no use for host threads (scanner.py:56-65)
        n_cpu = os.cpu_count() or 1
        n_threads = int(n_threads)
        if n_threads > n_cpu:
            logger.warning(f"Threads number exceed the number of CPUs, using {n_cpu} instead")
        self.n_threads = max(1, min(n_threads, n_cpu))
        self._starts, self._ends, self._sequences = [], [], []
        self._resident = None                # (ResidentGenome, chromosome indices) when extraction is on the device
        self._sq = None                      # the regions as a packed device set (0.375 B/base), kept between scan_motifs calls
        self._extract_seq(genome, regions)
        # frozen from here on: see _Frozen (the attributes are read-only properties, their lists refuse edits)
        self._starts, self._ends = _Frozen(self._starts), _Frozen(self._ends)
        if self._sequences is not None:
            self._sequences = _Frozen(self._sequences)

    @property
    def seq_starts(self):
        """0-based start of every scanned sequence on its chromosome (scanner.py:66)."""
        return self._starts

    @property
    def seq_ends(self):
        return self._ends

    @property
    def sequences(self):
        """Region sequences as strings (scanner.py:68).  With a ResidentGenome they are only
        materialised on demand (and only if the genome kept a host copy)."""
        if self._sequences is None and self._resident is None:        # a shuffled scanner: the bases were made on the device (to_strings copies the planes back)
            self._sequences = _Frozen(self._seqset().to_strings())
        if self._sequences is None:
            g, idx = self._resident
            self._sequences = _Frozen(g.fetch_sequence(g.names[c], lo, hi)
                                      for c, lo, hi in zip(idx, self.seq_starts, self.seq_ends))
        return self._sequences

    def _extract_seq(self, genome, regions):
        """Forward-strand sequence of every region (whole region, or a window of 2*(w//2) bp
        centred on the summit and clipped to the chromosome).  A `ResidentGenome` keeps the
        genome packed in HBM: then only coordinates are collected here and the regions are cut
        out on the device (ms_seqset_from_genome) instead of one fetch_sequence call per region."""
        logger.debug("Extracting sequences")
        whole = self.window_size <= 0
        resident = isinstance(genome, _lib.ResidentGenome)
        if resident and isinstance(regions, RegionArray):
            # a region list that is already arrays (regions.generate_control_regions): the same starts and ends by array arithmetic.
            # Only the chromosome names some region uses are looked up, as in the loop below.
            sizes = np.zeros(len(regions.chroms), dtype=np.int64)
            to_genome = np.zeros(len(regions.chroms), dtype=np.int32)
            for k in np.unique(regions.chrom_idx).tolist():
                to_genome[k] = genome.index[regions.chroms[k]]
                if not whole:
                    sizes[k] = genome.chrom_sizes[regions.chroms[k]]
            if whole:
                lo, hi = regions.start, regions.end
            else:
                lo = np.maximum(regions.summit - self.extend, 0)
                hi = np.minimum(regions.summit + self.extend, sizes[regions.chrom_idx])
            self._starts, self._ends = lo.tolist(), hi.tolist()
            self._resident = (genome, to_genome[regions.chrom_idx])
            self._sequences = None
            return
        chrom_idx = []
        for region in regions:
            if whole:
                lo, hi = region.start, region.end
            else:
                lo = max(region.summit - self.extend, 0)
                hi = min(region.summit + self.extend, genome.chrom_sizes[region.chrom])
            self._starts.append(lo)
            self._ends.append(hi)
            if resident:
                chrom_idx.append(genome.index[region.chrom])
            else:
                self._sequences.append(genome.fetch_sequence(region.chrom, lo, hi))
        if resident:
            self._resident = (genome, chrom_idx)
            self._sequences = None

    def _seqset(self):
        """The regions as a device sequence set (convert_seq, cscore.c:81-114: 2-bit codes + non-ACGT mask), made on the first scan
        and kept for the scanner's life -- the reference converts its strings again on every c_scan_motif call.  The regions are
        frozen after construction (`_Frozen`), so the cached set cannot go stale; `close()` releases it."""
        if self._sq is None:
            if self._resident is not None:
                g, idx = self._resident
                self._sq = g.extract(idx, self.seq_starts, self.seq_ends)
            elif self._sequences is None:
                raise RuntimeError("this shuffled scanner was closed before its sequences were read: its bases lived on the device only")
            else:
                self._sq = _lib.SeqSet.from_strings(self._sequences)
        return self._sq

    def shuffled(self, kind="dinuc", seed=0):
        """A Scanner over the same coordinates whose sequences are this scanner's, shuffled on the device (ms_seqset_shuffle): "mono" keeps
        the base composition, "dinuc" every dinucleotide count and both end bases of every run of ACGT; non-ACGT positions stay where they
        are, so every region keeps its count of valid windows.  The composition-matched control for `rank_sum`, `affinity_rank_sum`,
        `score_histogram`, `best_sites` and `scan_motifs` when there is no genomic one (sequences from a FASTA, a personal genome):
        `scanner.rank_sum(pwms, control=scanner.shuffled(seed=1))`.  The result does not depend on how the regions are sharded as long
        as each shard passes its own first index (`SeqSet.shuffled(..., seq_index_base)`); here the scanner is the whole set.  The new
        scanner owns its device set (it never takes the sweep or scan-once paths: there is no genome behind it); its `sequences` are
        copied back from the device on first use."""
        other = Scanner.__new__(Scanner)
        other.window_size, other.extend = self.window_size, self.extend
        other.strand, other.p_value, other.remove_dup, other.n_threads = self.strand, self.p_value, self.remove_dup, self.n_threads
        other._starts, other._ends = self._starts, self._ends
        other._resident = None
        other._sequences = None
        other._sq = self._seqset().shuffled(kind, seed)
        return other

    def close(self):
        """Release the device copy of the regions (also done when the scanner is collected)."""
        if self._sq is not None:
            self._sq.close()
            self._sq = None

    def _as_sweep(self):
        """(genome, chromosome index, begin, end, window, stride) if the regions are the windows of ONE fixed-stride
        sweep of one chromosome of a ResidentGenome, in order -- then ms_scan_sweep gives the identical result while
        scoring every base once; None otherwise."""
        if self._resident is None or len(self.seq_starts) < 2:
            return None
        g, idx = self._resident
        st = np.asarray(self.seq_starts, dtype=np.int64)
        en = np.asarray(self.seq_ends, dtype=np.int64)
        ci = np.asarray(idx, dtype=np.int64)
        window, stride = int(en[0] - st[0]), int(st[1] - st[0])
        if window < 1 or stride < 1 or (ci != ci[0]).any() or ((en - st) != window).any() or (np.diff(st) != stride).any():
            return None
        return g, int(ci[0]), int(st[0]), int(en[-1]), window, stride

    def _as_overlapping(self):
        """(genome, chromosome indices) if the regions lie on a ResidentGenome and overlap enough (their union is under half of
        their summed length: peaks +- window/2 much closer than the window, dense random controls, cli/scan.py:43-48, 76-86) for
        ms_scan_regions_once to pay: it scores the union once and hands every site to each region that holds it -- the identical
        result.  At half it breaks even with the per-region scan (profiles/archive/r02_scan_once_overlap.log): the hand-out re-keys and
        re-orders every site."""
        if self._resident is None or len(self.seq_starts) < 2:
            return None
        g, idx = self._resident
        total = int(np.sum(np.asarray(self.seq_ends, dtype=np.int64) - np.asarray(self.seq_starts, dtype=np.int64)))
        if total == 0 or _lib.union_bases(idx, self.seq_starts, self.seq_ends) > 0.5 * total:
            return None
        return g, idx

    # ------------------------------------------------------------------ scanning --

    def _marshal(self, pwms):
        pwms = list(pwms)
        cutoffs = []
        for pwm in pwms:
            try:
                cutoffs.append(pwm.cutoffs[self.p_value])
            except (TypeError, KeyError):
                raise ValueError(f"PWM has no motif score cutoff set for P-value {self.p_value!r}")
        matrices = [np.asarray(pwm.matrix, dtype=np.float64) for pwm in pwms]
        lengths = [pwm.length for pwm in pwms]
        return matrices, np.asarray(cutoffs, dtype=np.float64), lengths

    def _scan(self, pwms, with_tables=False):
        """One device scan (+ de-dup): (hits dict of the library's pinned arrays, n_regions_with_site, tables or None)."""
        matrices, cutoffs, lengths = self._marshal(pwms)
        logger.debug("Scanning motif PWMs")
        pw = _lib.PwmSet.from_matrices(matrices, cutoffs)
        sweep = self._as_sweep()
        overlapping = self._as_overlapping() if sweep is None else None
        if sweep is not None:
            g, chrom, begin, end, window, stride = sweep
            res = _lib.scan_sweep(pw, g, chrom, begin, end, window, stride, _STRAND_FLAG[self.strand])
        elif overlapping is not None:
            g, idx = overlapping
            res = _lib.scan_regions_once(pw, g, idx, self.seq_starts, self.seq_ends, _STRAND_FLAG[self.strand])
        else:
            res = _lib.scan(pw, self._seqset(), _STRAND_FLAG[self.strand])
        try:
            if self.remove_dup:
                res.dedup(pw)                      # scanner.py:156-193 on the device, order preserved
            h = res.hits(copy=False, motif=False)  # views of the library's pinned host buffers (they keep `res` alive)
            region_counts = res.region_counts()
            tables = res.site_tables(len(self.seq_starts)) if with_tables else None
        except BaseException:
            res.close()
            raise
        finally:
            pw.close()
        return h, region_counts, tables, res

    def scan_motifs_arrays(self, pwms, with_tables=False):
        """Flat result: dict with motif, region, start (genome coordinate), score, strand (1/2),
        motif_offsets -- ordered exactly like the nested lists scan_motifs returns.  with_tables adds
        the dense per-(motif, region) site count and maximum score (NaN = no site)."""
        h, region_counts, tables, res = self._scan(pwms, with_tables)
        starts = np.asarray(self.seq_starts, dtype=np.int64)
        n_pwms = len(h["motif_offsets"]) - 1
        out = {"motif": np.repeat(np.arange(n_pwms, dtype=np.int32), np.diff(h["motif_offsets"])), "region": h["seq_idx"],
               "start": (starts[h["seq_idx"]] + h["pos"]) if len(h["pos"]) else h["pos"],
               "score": h["score"], "strand": h["strand"], "motif_offsets": h["motif_offsets"],
               "n_regions_with_site": region_counts,      # de-dup never empties a region
               "_result": res}                            # owns the memory behind region / score / strand
        if tables is not None:
            out["n_sites"], out["max_score"] = tables      # what write_sites_table prints (io/__init__.py:23-33)
        return out

    def scan_batches(self, pwms, batch_regions=100_000, depth=2):
        """Generator over consecutive batches of regions, for region lists whose sequences / hit lists should not sit in
        memory at once: yields (r0, r1, arrays) with `arrays` as scan_motifs_arrays returns them for regions [r0, r1)
        ('region' holds the GLOBAL region index).  The batches go through an ms_stream: the upload + packing of one batch,
        the scan of the previous one and the copy-out of the one before overlap on the device.  Concatenated per motif
        (_lib.merge_hits) the batches are exactly the single-call result."""
        matrices, cutoffs, lengths = self._marshal(pwms)
        n = len(self.seq_starts)
        pw = _lib.PwmSet.from_matrices(matrices, cutoffs)
        starts = np.asarray(self.seq_starts, dtype=np.int64)
        bounds = [(r0, min(n, r0 + batch_regions)) for r0 in range(0, n, max(1, int(batch_regions)))]

        def arrays(r0, res):
            h = res.hits(copy=False)
            region = h["seq_idx"] + r0
            return {"motif": h["motif"], "region": region, "start": (starts[region] + h["pos"]) if len(region) else h["pos"],
                    "score": h["score"], "strand": h["strand"], "motif_offsets": h["motif_offsets"],
                    "n_regions_with_site": res.region_counts(), "_result": res}     # score / strand are views of the result's pinned block

        def batches():
            for r0, r1 in bounds:
                seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in self.sequences[r0:r1]]
                offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
                if seqs:
                    offsets[1:] = np.cumsum([len(b) for b in seqs])
                yield np.frombuffer(b"".join(seqs), dtype=np.uint8), offsets

        try:
            flags = _lib.MS_STREAM_DEDUP if self.remove_dup else 0
            if self._resident is not None:               # regions are cut on the device (ms_stream_submit_regions): nothing to upload
                g, idx = self._resident
                cuts = ((g, idx[r0:r1], self.seq_starts[r0:r1], self.seq_ends[r0:r1]) for r0, r1 in bounds)
                for (r0, r1), res in zip(bounds, _lib.scan_stream(pw, cuts, _STRAND_FLAG[self.strand], flags, depth)):
                    yield r0, r1, arrays(r0, res)
            else:
                for (r0, r1), res in zip(bounds, _lib.scan_stream(pw, batches(), _STRAND_FLAG[self.strand], flags, depth)):
                    yield r0, r1, arrays(r0, res)
        finally:
            pw.close()

    def count_regions_with_sites(self, pwms):
        """int64 [n_pwms]: the number of this scanner's regions that hold >= 1 site of each motif -- what
        `stats.motif_enrichment` computes from the nested lists (`sum(len(sites_by_region) > 0 ...)`, stats.py:29-31) and ALL the
        reference ever reads of the CONTROL regions' scan (cli/scan.py:81-89).  The hits stay on the device: no copy-out, no
        Python object per site.  (De-duplication never empties a region, so the count does not depend on remove_dup.)"""
        matrices, cutoffs, _ = self._marshal(pwms)
        pw = _lib.PwmSet.from_matrices(matrices, cutoffs)
        try:
            sweep = self._as_sweep()
            overlapping = self._as_overlapping() if sweep is None else None
            if sweep is not None:
                g, chrom, begin, end, window, stride = sweep
                res = _lib.scan_sweep(pw, g, chrom, begin, end, window, stride, _STRAND_FLAG[self.strand])
            elif overlapping is not None:
                g, idx = overlapping
                res = _lib.scan_regions_once(pw, g, idx, self.seq_starts, self.seq_ends, _STRAND_FLAG[self.strand])
            else:
                # nothing but the counts is read: the hits are counted where the fp64 stage left them -- no ordering, no site arrays
                res = _lib.scan(pw, self._seqset(), _STRAND_FLAG[self.strand], _lib.MS_SCAN_COUNTS_ONLY)
            try:
                return res.region_counts()
            finally:
                res.close()
        finally:
            pw.close()

    def best_sites(self, pwms):
        """The best-scoring window of every (motif, region) cell -- the dense matrix behind "max motif score per region", and how far
        below its cutoff a region without a site stays -- as a BestSiteArrays.  Every window is scored as scan_motifs scores it; the
        first window in the reference's order (start ascending, '+' before '-') keeps a tie.  Honours the scanner's `strand`;
        `p_value` and `remove_dup` have no meaning here (no cutoff is read, one window per cell is reported)."""
        matrices = [np.asarray(pwm.matrix, dtype=np.float64) for pwm in pwms]
        pw = _lib.PwmSet.from_matrices(matrices)
        try:
            res = _lib.scan_best(pw, self._seqset(), _STRAND_FLAG[self.strand])
            try:
                score, pos, strand = res.sites()
            finally:
                res.close()
        finally:
            pw.close()
        return BestSiteArrays(score, best_site_starts(pos, self.seq_starts), strand)

    def _scan_best(self, pw):
        return _lib.scan_best(pw, self._seqset(), _STRAND_FLAG[self.strand])

    def rank_sum(self, pwms, control, sel=None, sel_control=None):
        """Is each motif enriched in this scanner's regions against `control`'s (another Scanner), without choosing a cutoff?  The
        rank-sum comparison of the best score per region, as an enrich.RankSum (.auroc(), .z(), .p_value()).  Both region lists are
        scanned with ms_scan_best, each with its scanner's `strand`; both matrices stay on the device and are reduced there
        (ms_best_rank_sum) -- no matrix is copied.  sel / sel_control: one flag per region of either scanner (None: all of them)."""
        from . import enrich
        matrices = [np.asarray(pwm.matrix, dtype=np.float64) for pwm in pwms]
        pw = _lib.PwmSet.from_matrices(matrices)
        try:
            mine = self._scan_best(pw)
            try:
                theirs = control._scan_best(pw)
                try:
                    return enrich.rank_sum(mine, theirs, sel, sel_control)
                finally:
                    theirs.close()
            finally:
                mine.close()
        finally:
            pw.close()

    def _scan_best_dimodels(self, ms):
        return _lib.scan_best_dimodels(ms, self._seqset(), _STRAND_FLAG[self.strand])

    def best_sites_dimodels(self, models):
        """best_sites for first-order models (dimodel.DiModel objects or a dimodel.DiModelSet): the best-scoring window of every
        (model, region) cell as a BestSiteArrays (ms_scan_best_dimodels).  A window that holds a non-ACGT base has no score; the walk
        and the tie rule are best_sites'.  Honours the scanner's `strand`."""
        ms = _lib.DiModelSet.from_models(models)
        try:
            res = self._scan_best_dimodels(ms)
            try:
                score, pos, strand = res.sites()
            finally:
                res.close()
        finally:
            ms.close()
        return BestSiteArrays(score, best_site_starts(pos, self.seq_starts), strand)

    def rank_sum_dimodels(self, models, control, sel=None, sel_control=None):
        """rank_sum for first-order models: is each model enriched in this scanner's regions against `control`'s, by the best score per
        region and without a cutoff?  An enrich.RankSum.  Both region lists are scanned with ms_scan_best_dimodels, each with its
        scanner's `strand`; the matrices stay on the device and are reduced there (ms_best_rank_sum)."""
        from . import enrich
        ms = _lib.DiModelSet.from_models(models)
        try:
            mine = self._scan_best_dimodels(ms)
            try:
                theirs = control._scan_best_dimodels(ms)
                try:
                    return enrich.rank_sum(mine, theirs, sel, sel_control)
                finally:
                    theirs.close()
            finally:
                mine.close()
        finally:
            ms.close()

    def _scan_best_bipartite(self, pw, specs):
        return _lib.scan_best_bipartite(pw, specs, self._seqset(), _STRAND_FLAG[self.strand])

    def best_sites_bipartite(self, pwms, specs):
        """best_sites for bipartite motifs (bipartite.Bipartite specs over `pwms`: two half-sites with a spacer of gap_min .. gap_max
        bases): the best placement of every (spec, region) cell as a bipartite.BipartiteSites (ms_scan_best_bipartite) -- start is the
        leftmost base of the whole site, gap the winner's spacer length.  The halves are scored as best_sites scores them; the first
        placement in the walk's order (start ascending, '+' before '-', gap ascending) keeps a tie.  Honours the scanner's `strand`."""
        from . import bipartite
        matrices = [np.asarray(pwm.matrix, dtype=np.float64) for pwm in pwms]
        pw = _lib.PwmSet.from_matrices(matrices)
        try:
            res = self._scan_best_bipartite(pw, specs)
            try:
                score, pos, strand = res.sites()
                gap = res.gaps()
            finally:
                res.close()
        finally:
            pw.close()
        return bipartite.BipartiteSites(score, best_site_starts(pos, self.seq_starts), strand, gap)

    def rank_sum_bipartite(self, pwms, specs, control, sel=None, sel_control=None):
        """rank_sum for bipartite motifs: is each spec enriched in this scanner's regions against `control`'s, by the best score per
        region and without a cutoff?  An enrich.RankSum.  Both region lists are scanned with ms_scan_best_bipartite, each with its
        scanner's `strand`; the matrices stay on the device and are reduced there (ms_best_rank_sum)."""
        from . import enrich
        matrices = [np.asarray(pwm.matrix, dtype=np.float64) for pwm in pwms]
        pw = _lib.PwmSet.from_matrices(matrices)
        try:
            mine = self._scan_best_bipartite(pw, specs)
            try:
                theirs = control._scan_best_bipartite(pw, specs)
                try:
                    return enrich.rank_sum(mine, theirs, sel, sel_control)
                finally:
                    theirs.close()
            finally:
                mine.close()
        finally:
            pw.close()

    def count_regions_passing(self, pwms, cutoffs):
        """int64 [n_pwms][K]: the number of this scanner's regions that hold >= 1 site of each motif at each of its K cutoffs
        (cutoffs [n_pwms][K]) -- count_regions_with_sites at K cutoffs from ONE best-site scan (ms_best_count_passing) instead of K
        scans.  Honours `strand`; the PWMs' own cutoffs and `p_value` are not read."""
        matrices = [np.asarray(pwm.matrix, dtype=np.float64) for pwm in pwms]
        pw = _lib.PwmSet.from_matrices(matrices)
        try:
            res = self._scan_best(pw)
            try:
                return res.count_passing(cutoffs)
            finally:
                res.close()
        finally:
            pw.close()

    def _scan_affinity(self, pw, scale, max_n):
        return _lib.scan_affinity(pw, self._seqset(), _STRAND_FLAG[self.strand], scale, max_n)

    def affinity(self, pwms, scale=1.0, max_n=-1):
        """The total binding affinity of every (motif, region) cell -- the likelihood ratio exp(scale * raw score) summed over ALL
        windows of the region, the cutoff-free statistic that still sees a weak site repeated five times -- as an
        affinity.AffinityArrays (peak, sum, n_terms, log_mean; .log_sum(), .mean_odds()).  Every window is scored as scan_motifs scores
        it, nothing is normalised (the PWMs are natural-log odds: scale = 1.0; ln 2 for a log2 matrix).  max_n >= 0 leaves out the
        windows of more than max_n non-ACGT bases.  Honours the scanner's `strand`; `p_value` and `remove_dup` have no meaning here."""
        from . import affinity
        scale, max_n = affinity.check_args(scale, max_n)
        matrices = [np.asarray(pwm.matrix, dtype=np.float64) for pwm in pwms]
        pw = _lib.PwmSet.from_matrices(matrices)
        try:
            res = self._scan_affinity(pw, scale, max_n)
            try:
                return affinity.AffinityArrays(*res.cells())
            finally:
                res.close()
        finally:
            pw.close()

    def expected_counts(self, pwms, gamma=None, scale=1.0, max_n=-1):
        """The E-step of a motif refinement over this scanner's regions, without a cutoff: an em.ExpectedCounts -- per motif column the
        A, C, G, T weight under it over ALL windows, every window weighted by its posterior probability of being the site
        (ms_scan_affinity, then ms_affinity_expected_counts on its handle).  gamma: the fraction of regions that hold a site (ZOOPS);
        None: one site per region (OOPS).  Honours the scanner's `strand`, as `affinity` does."""
        from . import affinity, em
        scale, max_n = affinity.check_args(scale, max_n)
        prior = em.prior_logit_of(gamma)
        matrices = [np.asarray(pwm.matrix, dtype=np.float64) for pwm in pwms]
        pw = _lib.PwmSet.from_matrices(matrices)
        try:
            res = self._scan_affinity(pw, scale, max_n)
            try:
                return em.ExpectedCounts(*res.expected_counts(pw, self._seqset(), prior), [m.shape[1] for m in matrices])
            finally:
                res.close()
        finally:
            pw.close()

    def refine_motifs(self, pwms, iters=10, gamma=0.5, update_gamma=True, scale=1.0, max_n=-1, bg=None, pseudo=0.01):
        """em.refine of the PWMs' matrices over this scanner's regions, on the device: an em.Refinement (the matrices, the gamma values
        and the log-likelihood trace per iteration).  Honours the scanner's `strand`."""
        from . import affinity, em
        scale, max_n = affinity.check_args(scale, max_n)
        matrices = [np.asarray(pwm.matrix, dtype=np.float64) for pwm in pwms]
        em.check_gamma(gamma, len(matrices))
        return em.refine(matrices, self._seqset(), iters=iters, gamma=gamma, update_gamma=update_gamma, strand=_STRAND_FLAG[self.strand], scale=scale,
                         max_n=max_n, bg=bg, pseudo=pseudo, device=True)

    def affinity_rank_sum(self, pwms, control, sel=None, sel_control=None, scale=1.0, max_n=-1):
        """rank_sum with the region's mean likelihood ratio over all windows (affinity's log_mean) in place of its best score: an
        enrich.RankSum.  Both region lists are scanned with ms_scan_affinity, each with its scanner's `strand`; the planes stay on the
        device and are reduced there (ms_affinity_rank_sum).  A region without a term (shorter than the motif) ranks below every other."""
        from . import affinity, enrich
        scale, max_n = affinity.check_args(scale, max_n)
        if not isinstance(control, Scanner):
            raise ValueError("control must be a Scanner")
        for s, n in ((sel, len(self.seq_starts)), (sel_control, len(control.seq_starts))):
            if s is not None and np.shape(s) != (n,):
                raise ValueError(f"a selection must hold one flag per region ({n}), got shape {np.shape(s)}")
        matrices = [np.asarray(pwm.matrix, dtype=np.float64) for pwm in pwms]
        pw = _lib.PwmSet.from_matrices(matrices)
        try:
            mine = self._scan_affinity(pw, scale, max_n)
            try:
                theirs = control._scan_affinity(pw, scale, max_n)
                try:
                    return enrich.RankSum(*mine.rank_sum(theirs, sel, sel_control))
                finally:
                    theirs.close()
            finally:
                mine.close()
        finally:
            pw.close()

    def score_histogram(self, pwms, lo=0.0, hi=None, n_bins=1024, per_position=False):
        """The score distribution of ALL windows of the scanner's regions, per motif, as a scoredist.ScoreHistogram: n_bins equal bins over
        [lo, hi) plus a "below" and an "above" slot, every window scored as scan_motifs scores it and counted on the device
        (ms_scan_score_histogram).  One count per (window, strand of the scanner's `strand`), or with per_position one per window start
        (the greater strand: c_score's score of a position).  hi=None: the least double above 1.0, scaled so that a score of exactly
        1.0 falls in the last bin (scoredist.default_hi).  `p_value` and `remove_dup` have no meaning here; no window is dropped for its
        N bases.  From the histogram: ScoreHistogram.tail (sites at any cutoff), .p_value (empirical P-value of a site), .cutoffs."""
        from . import scoredist
        if hi is None:
            hi = scoredist.default_hi(lo, n_bins)
        matrices = [np.asarray(pwm.matrix, dtype=np.float64) for pwm in pwms]
        pw = _lib.PwmSet.from_matrices(matrices)
        try:
            counts = _lib.score_histogram(pw, self._seqset(), _STRAND_FLAG[self.strand], lo, hi, n_bins, per_position)
        finally:
            pw.close()
        return scoredist.ScoreHistogram.from_range(counts, lo, hi, n_bins)

    def score_distribution(self, pwms, order=0, n_bins=65536, pseudocount=1.0):
        """The ANALYTIC score distribution of the motifs under a Markov background of `order` counted on the scanner's own regions, as a
        pvalues.ScoreDistribution (ms_seqset_kmer_counts for the (order + 1)-mer counts, ms_pwmset_score_distribution for the
        distribution; the scanner's `strand`).  No window of the regions is scored: .p_value_bounds gives the P-value of a site,
        .cutoffs conservative cutoffs, from the matrix and the background alone."""
        from . import pvalues
        cond, init = pvalues.background_from_counts(self.kmer_counts(int(order) + 1, canonical=False), pseudocount)
        matrices = [np.asarray(pwm.matrix, dtype=np.float64) for pwm in pwms]
        return pvalues.score_distribution(matrices, cond, init, n_bins, _STRAND_FLAG[self.strand])

    def site_base_counts(self, pwms, flank=0, dinuc=False):
        """What the sites of a scan look like, as a sitestack.SiteStack: per motif and per column of the motif, with `flank` columns
        either side, how many sites have A, C, G, T there in the motif's orientation, a non-ACGT base, or lie outside the region there
        (ms_result_site_base_counts); dinuc adds the counts of the 16 base pairs of adjacent columns.  One scan of the scanner's own
        sequence set with its `strand` and `p_value`, de-duplicated if `remove_dup`, counted where it lies: no hit leaves the device.
        SiteStack.pfm(i) is the observed count matrix of motif i's sites."""
        from . import sitestack
        matrices, cutoffs, lengths = self._marshal(pwms)
        pw = _lib.PwmSet.from_matrices(matrices, cutoffs)
        try:
            sq = self._seqset()
            res = _lib.scan(pw, sq, _STRAND_FLAG[self.strand])
            try:
                if self.remove_dup:
                    res.dedup(pw)
                counts, di, n_sites = res.site_base_counts(pw, sq, int(flank), dinuc=dinuc)
            finally:
                res.close()
        finally:
            pw.close()
        return sitestack.SiteStack(counts, di, n_sites, np.asarray(lengths, dtype=np.int64), int(flank))

    def site_signal(self, pwms, track, flank=0, per_site=False):
        """A per-base signal track read over the sites of a scan, as a footprint.SiteSignal: per motif, strand and column of the motif,
        with `flank` columns either side and in the motif's orientation, the track summed over the sites whose column lies inside the
        region and the number of those sites (ms_result_site_signal); per_site adds every site's upstream, core and downstream sum.
        track: a footprint.Track (uploaded for the call) or a _lib.Track over the scanner's regions, in their order and of their lengths.
        One scan of the scanner's own sequence set with its `strand` and `p_value`, de-duplicated if `remove_dup`, read where it lies:
        no hit leaves the device."""
        from . import footprint
        matrices, cutoffs, lengths = self._marshal(pwms)
        pw = _lib.PwmSet.from_matrices(matrices, cutoffs)
        tr, tr_owned = None, False
        try:
            tr, tr_owned = footprint._track(track)
            res = _lib.scan(pw, self._seqset(), _STRAND_FLAG[self.strand])
            try:
                if self.remove_dup:
                    res.dedup(pw)
                total, cover, n_sites, ps = res.site_signal(pw, tr, int(flank), per_site=per_site)
                site_offsets = np.asarray(res.motif_offsets, dtype=np.int64).copy()
            finally:
                res.close()
        finally:
            if tr_owned:
                tr.close()
            pw.close()
        return footprint.SiteSignal(total, cover, n_sites, ps, site_offsets, np.asarray(lengths, dtype=np.int64), int(flank))

    def kmer_counts(self, k, canonical=True, sel=None):
        """The k-mer spectrum of the scanner's regions as a kmers.KmerCounts (ms_seqset_kmer_counts on the scanner's own device set, so a
        shuffled scanner or one over a personal genome counts its own bases): occ, the windows per k-mer; nseq, the regions that hold it
        at least once.  canonical folds a k-mer onto its reverse complement (a region set has no strand); pass canonical=False for
        KmerCounts.markov().  sel: one flag per region.  `strand`, `p_value` and `remove_dup` have no meaning here."""
        return self._seqset().kmer_counts(k, canonical=canonical, sel=sel)

    def kmer_enrichment(self, control, k, canonical=True):
        """The k-mers enriched in this scanner's regions against the control scanner's, counted HOMER's way (a region counts a k-mer at
        most once): a kmers.KmerEnrichment -- .top(n) lists the seeds, kmers.seed_matrix turns one into a PWM for the next scan.
        `control` is another Scanner: a genomic control, or `self.shuffled(...)`."""
        from . import kmers
        if not isinstance(control, Scanner):
            raise ValueError("control must be a Scanner")
        return kmers.enrichment(self.kmer_counts(k, canonical), control.kmer_counts(k, canonical))

    def scan_motifs(self, pwms):
        """motif_sites[n_pwms][n_regions] -> list[MotifSite] (scanner.py:89-132), as a read-only nested view over the
        device's flat hit arrays: a region's list is built when it is indexed (motifscan_amd/sites.py), so the call costs
        the scan + the copy-out whatever n_pwms x n_regions is.  `.to_lists()` gives the reference's real lists."""
        h, region_counts, _, res = self._scan(list(pwms))
        return MotifSites(h["motif_offsets"], h["seq_idx"], h["pos"], h["score"], h["strand"], self.seq_starts,
                          n_regions_with_site=region_counts, owner=res)


def make_motif_sites(sites, seq_starts):
    """Pooled [seq_idx, pos, score, strand] hits -> [n_pwms][n_seqs] lists of MotifSite in genome coordinates."""
    out = []
    for per_pwm in sites:
        buckets = [[] for _ in seq_starts]
        for seq_idx, pos, score, strand in per_pwm:
            buckets[seq_idx].append(MotifSite(seq_starts[seq_idx] + pos, score, "+" if strand == 1 else "-"))
        out.append(buckets)
    return out


def _walk_strand_in_given_order(sites, length):
    """One strand's sites of one region in the order the CALLER gave them: the survivor of each comparison meets the next
    site of the list; `next.start - current.start < length` also holds for a site that lies to the LEFT of the current one
    (scanner.py:156-168 does not sort).  Returns the kept sites in list order."""
    kept, cur = [], None
    for s in sites:
        if cur is None:
            cur = s
        elif s.start - cur.start < length:
            if not cur.score >= s.score:
                cur = s                                             # the later one scores strictly higher: it replaces the current site
        else:
            kept.append(cur)
            cur = s
    if cur is not None:
        kept.append(cur)
    return kept


def deduplicate_motif_sites(motif_sites, lengths):
    """Drop the lower-scoring one of two same-strand sites closer than the motif length (greedy walk over each strand's sites IN
    THE ORDER GIVEN, ties keep the earlier site); the result is ordered by start with '+' before '-' (scanner.py:156-193).
    Regions whose strands are start-sorted -- everything a scan produces -- go through the C routine the array path uses
    (ms_dedup_hits), all of them in one call; a region handed over in any other order is walked here, in its own order."""
    motif, region, start, score, strand = [], [], [], [], []
    out = [[[] for _ in per_pwm] for per_pwm in motif_sites]
    for m, (per_pwm, length) in enumerate(zip(motif_sites, lengths)):
        for r, sites in enumerate(per_pwm):
            fwd = [s for s in sites if s.strand == "+"]
            rev = [s for s in sites if s.strand != "+"]
            if all(a.start <= b.start for part in (fwd, rev) for a, b in zip(part, part[1:])):
                # (start asc, '+' first) inside a region is what the C routine wants; the stable merge keeps each strand's own order
                for s in sorted(fwd + rev, key=lambda s: s.start):
                    motif.append(m)
                    region.append(r)
                    start.append(s.start)
                    score.append(s.score)
                    strand.append(1 if s.strand == "+" else 2)
            else:
                kept = _walk_strand_in_given_order(fwd, length) + _walk_strand_in_given_order(rev, length)
                out[m][r] = sorted(kept, key=lambda s: s.start)
    n_pwms = len(motif_sites)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(np.asarray(motif, dtype=np.int64), minlength=n_pwms))]) \
        if n_pwms else np.zeros(1)
    keep = _lib.dedup_keep(offsets, list(lengths), region, start, np.asarray(score, dtype=np.float64), strand) \
        if motif else np.zeros(0, dtype=bool)
    for k in np.nonzero(keep)[0].tolist():
        out[motif[k]][region[k]].append(MotifSite(start[k], score[k], "+" if strand[k] == 1 else "-"))
    return out
