"""
motifscan_amd.annotation -- gene annotations: the surface of the reference's `motifscan.genome.annotation`
(genome/annotation.py) over per-chromosome arrays.

Same names, arguments and errors:
    Gene(chrom, tss, strand, name=None)      .promoter(upstream=2000, downstream=2000)        annotation.py:14-29
    Genes(path)                              len(), .fetch(chrom) -> list of Gene ([] for an unknown chromosome)   annotation.py:32-54
    RefGeneTxtParser(path).parse()           refGene txt rows -> Gene                          annotation.py:57-78
    read_gene_annotation(path)               annotation.py:81-82

What differs is the storage: a `Genes` keeps, per chromosome in order of first appearance, the TSS and strand of its genes in FILE
order as arrays (`chrom_offsets`, `tss`, `strand`: 1 '+', 2 '-'), because file order is what `dis_to_nearest_gene` walks and what
`random.choice` indexes.  `Genes.table()` is the device copy of those arrays (made on first use and kept), which
motifscan_amd.regions hands to the kernels.  `Genes.from_arrays` builds one without a file.
"""
import logging

import numpy as np

logger = logging.getLogger(__name__)

_STRAND_CODE = {"+": 1, "-": 2}
_STRAND_CHAR = {1: "+", 2: "-"}


class Gene:
    """One gene (transcript): chromosome, TSS, strand, name."""

    def __init__(self, chrom, tss, strand, name=None):
        if strand not in _STRAND_CODE:
            raise ValueError(f"invalid strand option: {strand!r}")
        self.chrom = chrom
        self.tss = int(tss)
        self.strand = strand
        self.name = name

    def promoter(self, upstream=2000, downstream=2000):
        """[tss - upstream, tss + downstream] in the gene's own direction."""
        left, right = (upstream, downstream) if self.strand == "+" else (downstream, upstream)
        return [self.tss - left, self.tss + right]

    def __repr__(self):
        return f"Gene({self.name}, {self.chrom}:{self.tss}{self.strand})"


class RefGeneTxtParser:
    """refGene txt rows: column 2 is the name, 3 the chromosome, 4 the strand, 5 txStart, 6 txEnd.  A gene's TSS is its txStart on
    the '+' strand and its txEnd on the '-' strand; any other strand is a ValueError."""

    _TSS_COLUMN = {"+": 4, "-": 5}

    def __init__(self, path):
        self.path = path

    def _rows(self):
        """(chromosome, tss, strand, name) of every row, in file order."""
        with open(self.path, "r") as fh:
            for row in fh:
                row = row.strip()
                cells = row.split()
                column = self._TSS_COLUMN.get(cells[3])
                if column is None:
                    raise ValueError(f"Invalid strand {cells[3]!r} detected at line: {row}")
                yield cells[2], int(cells[column]), cells[3], cells[1]

    def columns(self):
        """The file as four parallel lists in row order: chromosome, tss, strand code (1 '+', 2 '-'), name.  What Genes is made of."""
        chrom, tss, strand, names = [], [], [], []
        for c, t, s, name in self._rows():
            chrom.append(c)
            tss.append(t)
            strand.append(_STRAND_CODE[s])
            names.append(name)
        return chrom, tss, strand, names

    def parse(self):
        """The rows as Gene objects, one at a time; the rows in front of a bad one are yielded before it raises."""
        for c, t, s, name in self._rows():
            yield Gene(c, t, s, name)


class Genes:
    """A gene set, grouped by chromosome (indexed by first appearance), file order inside a chromosome."""

    def __init__(self, path):
        self.path = path
        self.read_genes()

    @classmethod
    def from_arrays(cls, chrom, tss, strand, names=None, path=None):
        """chrom: one chromosome name per gene, in file order; strand: '+' / '-' characters or the codes 1 / 2."""
        self = cls.__new__(cls)
        self.path = path
        strand = np.asarray(strand)
        if strand.dtype.kind in "US":
            strand = strand.astype(str)
            bad = ~np.isin(strand, ("+", "-"))
            if bad.any():
                raise ValueError(f"invalid strand option: {str(strand[bad][0])!r}")
            strand = np.where(strand == "+", 1, 2)
        self._set(list(chrom), np.asarray(tss, dtype=np.int64), strand.astype(np.int8), None if names is None else list(names))
        return self

    def _set(self, chrom, tss, strand, names):
        if not (len(chrom) == tss.size == strand.size) or (names is not None and len(names) != len(chrom)):
            raise ValueError("need one chromosome, tss and strand per gene")
        if strand.size and not np.isin(strand, (1, 2)).all():
            raise ValueError("strand codes must be 1 ('+') or 2 ('-')")
        self.chrom_names, self.index = [], {}
        code = np.zeros(len(chrom), dtype=np.int64)
        for i, c in enumerate(chrom):
            k = self.index.get(c)
            if k is None:
                k = self.index[c] = len(self.chrom_names)
                self.chrom_names.append(c)
            code[i] = k
        order = np.argsort(code, kind="stable")           # chromosome-major, file order kept inside a chromosome
        self.chrom_offsets = np.zeros(len(self.chrom_names) + 1, dtype=np.int64)
        np.cumsum(np.bincount(code, minlength=len(self.chrom_names)), out=self.chrom_offsets[1:])
        self.tss = np.ascontiguousarray(tss[order])
        self.strand = np.ascontiguousarray(strand[order])
        self.names = None if names is None else [names[i] for i in order.tolist()]
        self._fetched = {}
        self._table = None

    def read_genes(self):
        logger.debug(f"Loading genes from {self.path}")
        chrom, tss, strand, names = RefGeneTxtParser(self.path).columns()
        self._set(chrom, np.asarray(tss, dtype=np.int64), np.asarray(strand, dtype=np.int8), names)
        logger.debug(f"Loaded {len(self)} genes")

    def __len__(self):
        return int(self.chrom_offsets[-1])

    def chrom_range(self, chrom):
        """(lo, hi): the chromosome's genes are [lo, hi) of tss / strand; (0, 0) for an unknown chromosome."""
        k = self.index.get(chrom)
        return (0, 0) if k is None else (int(self.chrom_offsets[k]), int(self.chrom_offsets[k + 1]))

    def fetch(self, chrom):
        """The chromosome's genes in file order; [] for an unknown chromosome.  The list is made once and kept."""
        if chrom not in self.index:
            return []
        got = self._fetched.get(chrom)
        if got is None:
            lo, hi = self.chrom_range(chrom)
            got = self._fetched[chrom] = [Gene(chrom, t, _STRAND_CHAR[s], None if self.names is None else self.names[lo + i])
                                          for i, (t, s) in enumerate(zip(self.tss[lo:hi].tolist(), self.strand[lo:hi].tolist()))]
        return got

    def table(self):
        """The device handle of the arrays (_lib.GeneTable), made on first use and kept.  Making it needs the library, not a device."""
        if self._table is None:
            from . import _lib
            self._table = _lib.GeneTable(self.chrom_offsets, self.tss, self.strand)
        return self._table


def read_gene_annotation(path):
    return Genes(path)
