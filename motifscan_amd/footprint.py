"""
motifscan_amd.footprint -- a per-base SIGNAL read over the sites of a scan: ATAC / DNase cut counts, ChIP coverage, conservation or any
other per-base track in fixed point, summed on the device from the hit arrays of a result and a resident int32 track laid out like the
scanned regions (ms_sitesignal.hip).  The reference has no counterpart: it hands back nested site lists, and a footprint plot is then one
numpy slice per site and some 200 columns per slice.

    Track                             the track on the HOST: int32 values and the regions' offsets; nothing touches a device until
                                      site_signal uploads it (Track.upload() -> _lib.Track).  Constructors: from_arrays (one array per
                                      region), from_chrom_arrays (per-chromosome arrays cut by the regions), from_points (cut sites
                                      counted per base), from_intervals (bedGraph rows painted onto the regions), from_float (fixed
                                      point: rint(v * scale)).
    site_signal(motif_sites, pwms, track, flank=0, motifs=slice(None), per_site=False) -> SiteSignal
        per motif, strand and column of the motif (with `flank` columns either side), in the MOTIF's orientation: the track summed over
        the motif's sites whose column lies inside the region, and how many sites those are; with per_site=True also, per site, the sums
        over its upstream flank, core and downstream flank (ms_result_site_signal).
    SiteSignal.profile(i, strand)     int64 [W + 2 * flank], one strand or both folded
    SiteSignal.mean_profile(i)        float64: folded sum / folded cover -- a host division, as are depth and site_scores
    SiteSignal.depth(i)               mean over the flank columns minus mean over the core columns: > 0 is a footprint
    SiteSignal.site_scores(i)         per site: flank signal per covered flank column minus core signal per covered core column
    site_signal_host(...)             the same sums one site and one column at a time in plain Python ints: the definition, restated

`motif_sites` is what `sitestack.site_base_counts` accepts: a `MotifSites` (while it still owns its device result that result is read in
place, otherwise its flat arrays are uploaded) or the reference's nested lists, whose sites carry genome coordinates: pass the regions'
starts as `seq_starts` then.  The sums are exact int64 and additive over region shards.  There is no CPU path behind site_signal: without
a device it raises.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from .pairs import _pwmset, _rows, _runs
from .plot import _device_sites
from .sites import MotifSites
from .sitestack import _shifted

MAX_FLANK = 512

_INT32 = np.iinfo(np.int32)


def _region_fields(regions):
    chrom = [r.chrom for r in regions]
    start = np.fromiter((r.start for r in regions), dtype=np.int64, count=len(chrom))
    end = np.fromiter((r.end for r in regions), dtype=np.int64, count=len(chrom))
    if (end < start).any():
        raise ValueError("a region ends before it starts")
    offsets = np.zeros(len(chrom) + 1, dtype=np.int64)
    np.cumsum(end - start, out=offsets[1:])
    return chrom, start, end, offsets


def _as_int32(values, what="values"):
    a = np.asarray(values)
    if a.size == 0:
        return np.zeros(a.shape, dtype=np.int32)
    if a.dtype.kind not in "iub":
        raise ValueError(f"{what} must be integers (Track.from_float turns floats into fixed point)")
    if a.size and (a.min() < _INT32.min or a.max() > _INT32.max):
        raise ValueError(f"{what} do not fit int32")
    return a.astype(np.int32)


class Track:
    """int32 values [offsets[-1]] and int64 offsets [R + 1] on the host: one value per base of the regions, region after region."""

    def __init__(self, values, offsets):
        self.values = np.ascontiguousarray(_as_int32(values)).reshape(-1)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if self.offsets.ndim != 1 or self.offsets.size < 1 or self.offsets[0] != 0 or (np.diff(self.offsets) < 0).any():
            raise ValueError("offsets must hold n_regions + 1 entries, start at 0 and not decrease")
        if int(self.offsets[-1]) != self.values.size:
            raise ValueError("offsets[-1] must equal the number of values")

    @property
    def n_regions(self):
        return self.offsets.size - 1

    def region(self, r):
        return self.values[int(self.offsets[r]):int(self.offsets[r + 1])]

    @classmethod
    def from_arrays(cls, arrays):
        """One integer array per region, in the regions' order."""
        arrays = [_as_int32(a).reshape(-1) for a in arrays]
        offsets = np.zeros(len(arrays) + 1, dtype=np.int64)
        if arrays:
            np.cumsum([a.size for a in arrays], out=offsets[1:])
        return cls(np.concatenate(arrays) if arrays else np.zeros(0, dtype=np.int32), offsets)

    @classmethod
    def from_chrom_arrays(cls, chrom_arrays, regions):
        """{chrom: integer array over the whole chromosome} cut by the regions (objects with chrom, start, end); the part of a region
        that lies outside its chromosome's array reads 0."""
        chrom, start, end, offsets = _region_fields(regions)
        values = np.zeros(int(offsets[-1]), dtype=np.int32)
        cache = {}
        for r, c in enumerate(chrom):
            if c not in chrom_arrays:
                continue
            if c not in cache:
                cache[c] = _as_int32(chrom_arrays[c], f"the values of {c}").reshape(-1)
            src = cache[c]
            lo, hi = max(int(start[r]), 0), min(int(end[r]), src.size)
            if lo < hi:
                at = int(offsets[r]) + lo - int(start[r])
                values[at:at + hi - lo] = src[lo:hi]
        return cls(values, offsets)

    @classmethod
    def from_points(cls, chrom, pos, regions, weight=1):
        """Cut sites (chrom[i], pos[i]) counted per base of the regions, each adding weight (a scalar or one integer per point); a point
        inside several overlapping regions counts in each, one outside every region in none."""
        rchrom, start, end, offsets = _region_fields(regions)
        chrom, pos = np.asarray(chrom), np.asarray(pos, dtype=np.int64)
        weight = np.broadcast_to(np.asarray(weight, dtype=np.int64), pos.shape)
        total = np.zeros(int(offsets[-1]), dtype=np.int64)
        by_chrom = {}
        for r, c in enumerate(rchrom):
            by_chrom.setdefault(c, []).append(r)
        for c, rs in by_chrom.items():
            sel = chrom == c
            if not sel.any():
                continue
            p, w = pos[sel], weight[sel]
            order = np.argsort(p, kind="stable")
            p, w = p[order], w[order]
            for r in rs:
                i, j = np.searchsorted(p, [start[r], end[r]], side="left")
                if i < j:
                    np.add.at(total, int(offsets[r]) + p[i:j] - int(start[r]), w[i:j])
        return cls(_as_int32(total, "the summed weights"), offsets)

    @classmethod
    def from_intervals(cls, chrom, start, end, value, regions):
        """bedGraph rows (chrom[i], start[i], end[i], value[i]), half-open, painted onto the regions: a base takes the value of the LAST
        row that covers it, 0 without one; rows are clipped to the regions."""
        rchrom, rstart, rend, offsets = _region_fields(regions)
        chrom = np.asarray(chrom)
        start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
        value = _as_int32(value, "interval values")
        values = np.zeros(int(offsets[-1]), dtype=np.int32)
        rows_of = {}
        for i, c in enumerate(chrom.tolist()):
            rows_of.setdefault(c, []).append(i)
        for r, c in enumerate(rchrom):
            for i in rows_of.get(c, ()):
                lo, hi = max(int(start[i]), int(rstart[r])), min(int(end[i]), int(rend[r]))
                if lo < hi:
                    at = int(offsets[r]) - int(rstart[r])
                    values[at + lo:at + hi] = value[i]
        return cls(values, offsets)

    @classmethod
    def from_float(cls, values, offsets, scale):
        """Fixed point: np.rint(values * scale), which rounds halves to even.  Values that are not finite or do not fit int32 after
        scaling are refused."""
        v = np.rint(np.asarray(values, dtype=np.float64) * float(scale))
        if v.size and (not np.isfinite(v).all() or v.min() < _INT32.min or v.max() > _INT32.max):
            raise ValueError("the scaled values do not fit int32")
        return cls(v.astype(np.int64), offsets)

    def upload(self):
        """The track on the current device: a _lib.Track (close it when done)."""
        return _lib.Track.from_values(self.values, self.offsets)


def _track(track):
    """(_lib.Track, ours to close)"""
    if isinstance(track, _lib.Track):
        return track, False
    if isinstance(track, Track):
        return track.upload(), True
    raise TypeError("track must be a footprint.Track or a _lib.Track")


_SiteSignal = namedtuple("SiteSignal", ["sum", "cover", "n_sites", "per_site", "site_offsets", "widths", "flank"])


class SiteSignal(_SiteSignal):
    """sum, cover int64 [rows][2][C], C = the scan's widest motif + 2 * flank: per strand ('+' 0, '-' 1) and column j of row i's motif
    (column flank + c is motif column c; columns from widths[i] + 2 * flank on are unused and zero) the track summed over the sites whose
    column lies inside the region, and the number of those sites; n_sites int64 [rows][2]; per_site int64 [n][3] or None: upstream, core
    and downstream sum of every site of the selected rows, row i's sites at site_offsets[i] .. site_offsets[i + 1] in the result's hit
    order; widths int64 [rows]; flank.  The means below are host float arithmetic on these integers."""
    __slots__ = ()

    def _ncol(self, i):
        return int(self.widths[i]) + 2 * self.flank

    def profile(self, i, strand=None):
        """int64 [W + 2 * flank]: row i's sums, strand None (both folded), '+' / 0 or '-' / 1."""
        row = self.sum[i, :, :self._ncol(i)]
        if strand is None:
            return row[0] + row[1]
        return row[{"+": 0, "-": 1}.get(strand, strand)].copy()

    def mean_profile(self, i):
        """float64 [W + 2 * flank]: folded sum / folded cover, 0 where no site covers the column."""
        n = self._ncol(i)
        s = (self.sum[i, 0, :n] + self.sum[i, 1, :n]).astype(np.float64)
        c = (self.cover[i, 0, :n] + self.cover[i, 1, :n]).astype(np.float64)
        return np.divide(s, c, out=np.zeros(n), where=c > 0)

    def depth(self, i):
        """Mean of the mean profile over the 2 * flank flank columns minus its mean over the W core columns (0.0 with flank 0)."""
        if self.flank == 0:
            return 0.0
        m, f, W = self.mean_profile(i), self.flank, int(self.widths[i])
        return float((m[:f].sum() + m[f + W:].sum()) / (2 * f) - m[f:f + W].mean())

    def site_scores(self, i, pos=None, lengths=None):
        """float64 per site of row i: (upstream + downstream) / flank columns covered minus core / W.  The flank columns a site covers
        are a closed form of its position: pass pos and lengths (per site: start within the region, the region's length) for sites
        whose flanks leave their region; without them every site is taken to cover all 2 * flank."""
        if self.per_site is None:
            raise ValueError("made without per_site")
        if self.flank == 0:
            raise ValueError("site scores need flank > 0")
        ps = self.per_site[int(self.site_offsets[i]):int(self.site_offsets[i + 1])].astype(np.float64)
        W, f = int(self.widths[i]), self.flank
        if pos is None:
            n_flank = np.full(len(ps), 2.0 * f)
        else:
            pos, lengths = np.asarray(pos, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
            n_flank = (np.minimum(pos, f) + np.minimum(lengths - pos - W, f)).astype(np.float64)      # the same on either strand
        flank_mean = np.divide(ps[:, 0] + ps[:, 2], n_flank, out=np.zeros(len(ps)), where=n_flank > 0)
        return flank_mean - ps[:, 1] / W


def site_signal_host(motif_offsets, seq_idx, pos, strand, widths, values, offsets, flank):
    """The definition of ms_result_site_signal restated one site and one column at a time in plain Python ints: hit arrays in ms_result
    order (strand 1 '+', 2 '-'), widths [P], values and offsets as a Track holds them.  Returns a SiteSignal over all P motifs with
    per_site."""
    widths = np.asarray(widths, dtype=np.int64)
    P, flank = len(widths), int(flank)
    if len(motif_offsets) != P + 1:
        raise ValueError("need motif_offsets[P + 1]")
    if not 0 <= flank <= MAX_FLANK:
        raise ValueError(f"flank must be in [0, {MAX_FLANK}]")
    offs = [int(x) for x in offsets]
    R = len(offs) - 1
    vals = np.asarray(values).tolist()
    C = (int(widths.max()) if P else 0) + 2 * flank
    total = [[[0] * C for _ in range(2)] for _ in range(P)]
    cover = [[[0] * C for _ in range(2)] for _ in range(P)]
    n_sites = [[0, 0] for _ in range(P)]
    per_site = []
    for m in range(P):
        W = int(widths[m])
        for k in range(int(motif_offsets[m]), int(motif_offsets[m + 1])):
            r, p, s = int(seq_idx[k]), int(pos[k]), int(strand[k]) - 1
            if not 0 <= r < R:
                raise ValueError(f"hit {k}: region {r} outside [0, {R})")
            L = offs[r + 1] - offs[r]
            if p < 0 or p + W > L:
                raise ValueError(f"hit {k}: the site does not lie inside its region")
            n_sites[m][s] += 1
            three = [0, 0, 0]
            for j in range(W + 2 * flank):
                q = p + W - 1 + flank - j if s else p - flank + j
                if 0 <= q < L:
                    v = vals[offs[r] + q]
                    total[m][s][j] += v
                    cover[m][s][j] += 1
                    three[0 if j < flank else 1 if j < flank + W else 2] += v
            per_site.append(three)
    return SiteSignal(np.array(total, dtype=np.int64).reshape(P, 2, C), np.array(cover, dtype=np.int64).reshape(P, 2, C),
                      np.array(n_sites, dtype=np.int64).reshape(P, 2), np.array(per_site, dtype=np.int64).reshape(-1, 3),
                      np.asarray(motif_offsets, dtype=np.int64) - int(motif_offsets[0]), widths, flank)


def site_signal(motif_sites, pwms, track, flank=0, motifs=slice(None), per_site=False, seq_starts=None):
    """SiteSignal of the motifs selected by `motifs` (a slice or motif indices).  pwms: the scan's PWMs (their widths lay out the
    columns) -- a _lib.PwmSet, matrices [4][W] or objects with a .matrix; track: a Track over the scanned regions (uploaded for the
    call) or a _lib.Track already resident; seq_starts: for nested lists only, the regions' starts in the coordinates the sites carry
    (default 0)."""
    if seq_starts is not None and not isinstance(motif_sites, MotifSites):
        motif_sites = _shifted(motif_sites, seq_starts)
    res, _, owned = _device_sites(motif_sites)
    pw, pw_owned, tr, tr_owned = None, False, None, False
    try:
        pw, pw_owned = _pwmset(pwms)
        tr, tr_owned = _track(track)
        rows = _rows(motifs, res.n_pwms)
        flank = int(flank)
        if not len(rows):                                        # the library still checks the other arguments
            res.site_signal(pw, tr, flank, 0, 0, per_site=per_site)
        parts = [res.site_signal(pw, tr, flank, int(rows[i]), int(rows[j - 1]) + 1, per_site=per_site) for i, j in _runs(rows)]
        widths = np.asarray(pw.widths, dtype=np.int64)
        C = (int(widths.max()) if len(widths) else 0) + 2 * flank
        cat = lambda i, shape: np.concatenate([p[i] for p in parts]) if parts else np.zeros(shape, dtype=np.int64)
        mo = np.asarray(res.motif_offsets, dtype=np.int64)
        site_offsets = np.concatenate(([0], np.cumsum(mo[rows + 1] - mo[rows]))).astype(np.int64)
        return SiteSignal(cat(0, (0, 2, C)), cat(1, (0, 2, C)), cat(2, (0, 2)), cat(3, (0, 3)) if per_site else None, site_offsets,
                          widths[rows], flank)
    finally:
        if tr_owned:
            tr.close()
        if pw_owned:
            pw.close()
        if owned:
            res.close()
