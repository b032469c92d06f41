"""Stage C's side outputs: what is filled from the tokenised records beside the profile.

A family (COVERAGE, DEPTH, IDENTITY, VARIANTS) is a descriptor: its flags, the side array of a batch it reads, its refusals, its header,
what it holds on the device, and how its device accumulator is opened and turned into the file's block.  ASSIGNMENTS
(--read_assignments) shares only the flag test, the refusal and the header: its rows come from stage C itself.  --consensus
(metalign_amd/consensus.py) is no family of its own: it reads VARIANTS' accumulator and opens it by itself too, and so do --ani and
--vcf (metalign_amd/refdiff.py), which compare it with the reference FASTA parsed on the device (metalign_amd/refseq.py).

SideOutputs is the families wanted for ONE input file.  map_and_profile opens it, feeds it the records and closes it; the
order is always coverage, depth, identity, variants, and whatever was opened is freed on every way out.

--side_reads unique (metalign_amd/side_reads.py is the definition): the accumulators are fed a copy of the records in which every
record that is not unique evidence for its taxon carries FLAG 2048 (mg_records_mask_unique_dev), the bit by which none of them
counts a record.  That needs stage C's verdicts, so the records are fed from inside stage C instead of before it.
"""
import os
import sys

import numpy as np

from . import _hip, assignments, consensus, coverage, depth, identity, refdiff, refseq, side_reads, variants


def _flag(args, name):
    return getattr(args, name, 'NONE') not in (None, 'NONE')  # (callers build Namespaces without it)


def reads_mode(args):
    """--side_reads: 'all' (the default) or 'unique'."""
    return getattr(args, 'side_reads', 'all')  # (callers build Namespaces without it)


def source_label(args, path):
    """The `source=` of a block: the path only where there is more than one input file."""
    return path if len(getattr(args, 'infiles', [])) > 1 else None


def lengths_array(lengths, acc_index):
    """{accession: length} -> uint64[accession row]."""
    arr = np.zeros(len(acc_index), dtype=np.uint64)
    for a, i in acc_index.items():
        arr[i] = lengths[a]
    return arr


class _Flags:
    """A group of flags that ask for one output: the test, the refusals and the header."""
    flags = ()
    refuse_world = refuse_paf = None  # (None: not refused)

    def wanted(self, args):
        return any(_flag(args, f) for f in self.flags)

    def refusal(self, args, what):
        """The exit text for more than one process (what = 'world') or a PAF input ('paf'); None: not refused."""
        return getattr(self, 'refuse_' + what)


class _Assignments(_Flags):
    flags = ('read_assignments',)
    # (the records the ranks gather on rank 0 carry no names)
    refuse_world = 'Error: --read_assignments runs in one process on one GPU; start it without torch.distributed.run.'

    def write_header(self, args):
        assignments.write_assignments(args.read_assignments, [])  # the header; every input file appends its rows


class _Family(_Flags):
    """side: the side array of a batch it reads ('places' / 'edits' / 'bases': the entries and their pool).  nomem: the exit text when the device refuses the memory,
    with the MB figure of nomem_mb."""
    side = nomem = None

    def paths(self, args):
        """The files it writes."""
        return [getattr(args, f) for f in self.flags if _flag(args, f)]

    def open(self, args, hip, lengths, acc_index):
        """The device accumulator for one input file (lengths: coverage.lengths_of — the file's @SQ lines over db_info's)."""
        try:
            return self._open(args, hip, lengths, acc_index)
        except _hip.HipError as e:
            if e.code != _hip.ERR_NOMEM:
                raise
            sys.exit(self.nomem % self.nomem_mb(args, lengths, acc_index))


class _Coverage(_Family):
    flags, side = ('coverage',), 'places'
    refuse_world = 'Error: --coverage runs in one process on one GPU; start it without torch.distributed.run.'
    refuse_paf = 'Error: --coverage needs SAM or BAM alignments: a PAF line has no POS and CIGAR columns.'
    nomem = 'Error: --coverage keeps one bit per reference base on the GPU; %d MB for this database do not fit.'

    def write_header(self, args):
        coverage.write_coverage(args.coverage)  # the column header; every input file appends its block

    def device_bytes(self, args, lengths, nacc, nrec):
        return sum(lengths.values()) // 8  # one bit per reference base

    def nomem_mb(self, args, lengths, acc_index):
        return int(lengths_array(lengths, acc_index).sum()) >> 23

    def _open(self, args, hip, lengths, acc_index):
        return hip.coverage(lengths_array(lengths, acc_index))

    def close(self, args, source, lengths, dev, acc_index, acc2info, taxid2info):
        """The device's sums -> the file's block."""
        try:
            aln, bases, covered, unplaced = dev.result()
        finally:
            dev.free()
        names = {i: a for a, i in acc_index.items()}
        per = {names[r]: [int(aln[r]), int(bases[r]), int(covered[r])] for r in np.flatnonzero(aln).tolist()}  # (the rows that are hit)
        self.append(args, source, coverage.Coverage(lengths, per, unplaced), acc2info, taxid2info)

    def append(self, args, source, cov, acc2info, taxid2info):
        coverage.write_coverage(args.coverage, coverage.rows(cov, acc2info, taxid2info), cov.unplaced, source=source_label(args, source),
                                append=True)

    def append_from_definition(self, args, path, lines, acc2info, taxid2info):
        self.append(args, path, coverage.coverage(lines, acc2info, args.pct_id), acc2info, taxid2info)


class _Depth(_Family):
    """--depth or --depth_windows: either one asks for the per-base depth."""
    flags, side = ('depth', 'depth_windows'), 'places'
    refuse_world = 'Error: --depth and --depth_windows run in one process on one GPU; start it without torch.distributed.run.'
    refuse_paf = 'Error: --depth and --depth_windows need SAM or BAM alignments: a PAF line has no POS and CIGAR columns.'
    nomem = 'Error: --depth keeps four bytes per reference base on the GPU; %d MB for this database do not fit.'

    def write_header(self, args):
        if _flag(args, 'depth'):
            depth.write_depth(args.depth)
        if _flag(args, 'depth_windows'):
            depth.write_windows(args.depth_windows)

    @staticmethod
    def window(args):
        return int(getattr(args, 'depth_window_size', 1000)) if _flag(args, 'depth_windows') else 0

    def device_bytes(self, args, lengths, nacc, nrec):
        """4 B per reference base and accession, 12 B per window, a 32 KB histogram row per accession that is hit (at most one per
        record)."""
        window = self.window(args)
        total = sum(lengths.values())
        nwin = sum((n + window - 1) // window for n in lengths.values()) if window else 0
        return 4 * (total + len(lengths)) + 12 * nwin + 8 * _hip.DEPTH_BINS * min(len(lengths), nrec)

    def nomem_mb(self, args, lengths, acc_index):
        return self.device_bytes(args, lengths, len(acc_index), 0) >> 20

    def _open(self, args, hip, lengths, acc_index):
        return hip.depth(lengths_array(lengths, acc_index), self.window(args))

    def close(self, args, source, lengths, dev, acc_index, acc2info, taxid2info):
        """The device's histogram rows and windows -> the file's blocks."""
        try:
            aln, unplaced, hist, win = dev.result()
        finally:
            dev.free()
        names = {i: a for a, i in acc_index.items()}
        per = {names[r]: [int(aln[r]), H] for r, H in hist.items()}
        windows = {names[r]: w for r, w in win.items()}
        self.append(args, source, depth.Depth(lengths, per, unplaced, dev.window, windows), acc2info, taxid2info)

    def append(self, args, source, dep, acc2info, taxid2info):
        source = source_label(args, source)
        if _flag(args, 'depth'):
            depth.write_depth(args.depth, depth.rows(dep, acc2info, taxid2info), dep.unplaced, source=source, append=True)
        if _flag(args, 'depth_windows'):
            depth.write_windows(args.depth_windows, depth.window_rows(dep, acc2info), source=source, append=True)

    def append_from_definition(self, args, path, lines, acc2info, taxid2info):
        self.append(args, path, depth.depth(lines, acc2info, args.pct_id, self.window(args)), acc2info, taxid2info)


class _Identity(_Family):
    flags, side = ('identity',), 'edits'
    refuse_world = 'Error: --identity runs in one process on one GPU; start it without torch.distributed.run.'
    refuse_paf = 'Error: --identity needs SAM or BAM alignments: the NM:i: and cg:Z: tags of a PAF line are not read.'
    nomem = 'Error: --identity keeps 1001 bins of eight bytes per accession on the GPU; %d MB for this database do not fit.'

    def write_header(self, args):
        identity.write_identity(args.identity)

    def device_bytes(self, args, lengths, nacc, nrec):
        """1001 bins of 8 B and three sums per accession, 8 B of edit per record (and as much again where a collation permutes
        them)."""
        return 8 * (_hip.IDENTITY_BINS + 3) * nacc + 16 * nrec

    def nomem_mb(self, args, lengths, acc_index):
        return self.device_bytes(args, lengths, len(acc_index), 0) >> 20

    def _open(self, args, hip, lengths, acc_index):
        return hip.identity(len(acc_index))

    def close(self, args, source, lengths, dev, acc_index, acc2info, taxid2info):
        """The device's sums and histogram rows -> the file's block."""
        try:
            aln, cols, eds, unscored, hist = dev.result()
        finally:
            dev.free()
        names = {i: a for a, i in acc_index.items()}
        per = {names[r]: [int(aln[r]), int(cols[r]), int(eds[r]), H] for r, H in hist.items()}
        self.append(args, source, identity.Identity(per, unscored), acc2info, taxid2info)

    def append(self, args, source, idn, acc2info, taxid2info):
        identity.write_identity(args.identity, identity.rows(idn, acc2info, taxid2info), idn.unscored, source=source_label(args, source),
                                append=True)

    def append_from_definition(self, args, path, lines, acc2info, taxid2info):
        self.append(args, path, identity.identity(lines, acc2info, args.pct_id), acc2info, taxid2info)


class _Variants(_Family):
    """--variants or --variant_sites: either one asks for the per-site allele counts.  --consensus (metalign_amd/consensus.py), --ani
    and --vcf (metalign_amd/refdiff.py) read the same accumulator and open it by themselves too: they are no members of `flags` —
    the refusal texts of the family — but of wanted(), each with refusal texts of its own."""
    flags, side = ('variants', 'variant_sites'), 'bases'
    riders = ('consensus', 'ani', 'vcf')
    refuse_world = 'Error: --variants and --variant_sites run in one process on one GPU; start it without torch.distributed.run.'
    refuse_paf = 'Error: --variants and --variant_sites need SAM or BAM alignments: a PAF line has no CIGAR and SEQ columns.'
    refuse_world_consensus = 'Error: --consensus runs in one process on one GPU; start it without torch.distributed.run.'
    refuse_paf_consensus = 'Error: --consensus needs SAM or BAM alignments: a PAF line has no CIGAR and SEQ columns.'
    refuse_world_ani = 'Error: --ani runs in one process on one GPU; start it without torch.distributed.run.'
    refuse_paf_ani = 'Error: --ani needs SAM or BAM alignments: a PAF line has no CIGAR and SEQ columns.'
    refuse_world_vcf = 'Error: --vcf runs in one process on one GPU; start it without torch.distributed.run.'
    refuse_paf_vcf = 'Error: --vcf needs SAM or BAM alignments: a PAF line has no CIGAR and SEQ columns.'
    refuse_no_reference = ('Error: --ani and --vcf compare the reads with the FASTA they were aligned to: give it with --reference '
                           '(or --db).')
    refuse_reference_missing = 'Error: the reference FASTA of --ani and --vcf does not exist: %s'
    refuse_vcf_files = ('Error: --vcf takes one input file: a VCF has no place for a block per file. Run the files one by one, '
                        'each with its own --vcf.')
    nomem = 'Error: --variants keeps sixteen bytes per reference base on the GPU; %d MB for this database do not fit.'
    _reference = None  # (path, the lengths' bytes, RefSeq): parsed once per run, reused while the lengths are the same

    def wanted(self, args):
        return _Family.wanted(self, args) or any(_flag(args, f) for f in self.riders)

    def refusal(self, args, what):
        """A rider as the family's only flag is refused under its own name (the first of them that was given)."""
        if _Family.wanted(self, args):
            return getattr(self, 'refuse_' + what)
        return getattr(self, 'refuse_%s_%s' % (what, next(f for f in self.riders if _flag(args, f))))

    def paths(self, args):
        """... and --ani's, a TSV with the `#reads` line of the others."""
        return _Family.paths(self, args) + ([args.ani] if _flag(args, 'ani') else [])

    @staticmethod
    def diffed(args):
        return _flag(args, 'ani') or _flag(args, 'vcf')

    @staticmethod
    def reference(args):
        """--reference, or by default the database FASTA the aligner gets (--db); None where there is neither."""
        ref = getattr(args, 'reference', 'AUTO')
        if ref not in (None, 'AUTO', 'NONE'):
            return ref
        db = getattr(args, 'db', 'NONE')
        return db if db not in (None, 'NONE') else None

    def check_reference(self, args):
        """The refusals of --ani / --vcf that need no GPU.  (`metalign` has no --db: its stages write temp_dir/cmashed_db.fna, which
        is wired to args.db after this check and exists by the time stage C opens.)"""
        if not self.diffed(args):
            return
        wired_later = hasattr(args, 'reads') and not hasattr(args, 'db') and getattr(args, 'reference', 'AUTO') == 'AUTO'
        if not wired_later:
            ref = self.reference(args)
            if ref is None:
                sys.exit(self.refuse_no_reference)
            if not os.path.isfile(ref):
                sys.exit(self.refuse_reference_missing % ref)
        if _flag(args, 'vcf') and len(getattr(args, 'infiles', ())) > 1:
            sys.exit(self.refuse_vcf_files)

    @staticmethod
    def params(args):
        return variants.params(getattr(args, 'variant_min_depth', 5), getattr(args, 'variant_min_count', 2),
                               getattr(args, 'variant_min_freq', 0.05))

    @staticmethod
    def min_called(args):
        """--consensus_min_called in parts per thousand; ValueError out of range."""
        return consensus.min_called_permille(getattr(args, 'consensus_min_called', 0.0))

    @staticmethod
    def iupac(args):
        return getattr(args, 'consensus_ambiguity', 'major') == 'iupac'

    def write_header(self, args):
        p = self.params(args)
        if _flag(args, 'variants'):
            variants.write_variants(args.variants, p)
        if _flag(args, 'variant_sites'):
            variants.write_sites(args.variant_sites, p)
        if _flag(args, 'consensus'):
            consensus.write_consensus(args.consensus)  # (an empty file: FASTA has no comment lines)
        if _flag(args, 'ani'):
            refdiff.write_ani(args.ani, p)
        if _flag(args, 'vcf'):
            open(args.vcf, 'w').close()  # (the one input file writes it whole: its header names the file's contigs)

    def device_bytes(self, args, lengths, nacc, nrec):
        """16 B per reference base and five sums per accession; per record a 16 B entry (and as much again where a collation
        permutes them) and the pool's 4-bit codes — 75 B for a 150-base read, reckoned as 80 B with the entry.  --consensus: a slab
        of text.  --ani / --vcf: one byte per reference base, four sums per accession and, while it is parsed, the FASTA text (a
        .gz reckoned at four times its size) with 40 B of line index per 60 of it."""
        need = 16 * sum(lengths.values()) + 40 * nacc + 16 * nrec + 80 * nrec
        if self.diffed(args):
            need += sum(lengths.values()) + 32 * nacc
            ref = self.reference(args)
            if ref is not None and os.path.isfile(ref) and self._reference_for(ref, lengths) is None:
                text = os.path.getsize(ref) * (4 if ref.endswith('.gz') else 1)
                need += text + 40 * (text // 60 + 1)
        if _flag(args, 'consensus'):
            need += min(consensus.SLAB_BYTES, sum(consensus.text_bytes(n) for n in lengths.values()))
        return need

    def nomem_mb(self, args, lengths, acc_index):
        return self.device_bytes(args, lengths, len(acc_index), 0) >> 20

    def _open(self, args, hip, lengths, acc_index):
        return hip.variants(lengths_array(lengths, acc_index))

    def close(self, args, source, lengths, dev, acc_index, acc2info, taxid2info):
        """The device's sums and polymorphic sites -> the files' blocks."""
        p = self.params(args)
        try:
            aln, call, poly, pairs, disc, unpiled, sites = dev.result(*p)
            if _flag(args, 'consensus'):
                self.write_consensus_from(args, source, lengths, dev, acc_index, acc2info, aln, call, poly)
            if self.diffed(args):
                self.append_diff(args, source, self.diff_from(args, lengths, dev, acc_index, acc2info, aln, call, unpiled), acc2info,
                                 taxid2info)
        finally:
            dev.free()
        if not _Family.wanted(self, args):
            return
        names = {i: a for a, i in acc_index.items()}
        per = {a: [int(aln[i]), int(call[i]), int(poly[i]), int(pairs[i]), int(disc[i])] for a, i in acc_index.items() if aln[i]}
        # (the device orders the sites by accession row; the file by db_info's order, which is the rows' where db_info has no
        # accession twice)
        order = {a: k for k, a in enumerate(acc2info)}
        rows = sorted(((names[int(s['acc'])], int(s['pos0']), tuple(int(x) for x in s['n'])) for s in sites),
                      key=lambda s: (order[s[0]], s[1]))
        self.append(args, source, variants.Variants(lengths, per, rows, unpiled), acc2info, taxid2info)

    def write_consensus_from(self, args, source, lengths, dev, acc_index, acc2info, aln, call, poly):
        """--consensus from the open accumulator: the accessions that are written, in db_info order; their text fetched in slabs of
        consecutive rows of up to consensus.SLAB_BYTES (half the rows again, down to one, where the device has no room for a slab),
        every record's header and its slice of the slab straight to the file."""
        p, M, iupac = self.params(args), self.min_called(args), self.iupac(args)
        unique, label = reads_mode(args) == 'unique', source_label(args, source)
        accs = [a for a in acc2info if aln[acc_index[a]] and consensus.written(lengths[a], int(call[acc_index[a]]), M)]
        sizes = [consensus.text_bytes(lengths[a]) for a in accs]
        todo = consensus.slabs(sizes)
        with open(args.consensus, 'ab') as out:
            while todo:
                first, end = todo.pop(0)
                try:
                    text = dev.consensus([acc_index[a] for a in accs[first:end]], p.min_depth, p.min_count, p.permille, iupac,
                                         consensus.LINE_WIDTH)
                except _hip.HipError as e:
                    if e.code != _hip.ERR_NOMEM or end - first < 2:
                        raise
                    mid = (first + end) // 2
                    todo[:0] = [(first, mid), (mid, end)]
                    continue
                at = 0
                for a, size in zip(accs[first:end], sizes[first:end]):
                    i = acc_index[a]
                    out.write(consensus.header_line(a, acc2info[a][1], lengths[a], int(aln[i]), int(call[i]), int(poly[i]), p, iupac,
                                                    unique, label).encode('utf-8'))
                    out.write(text[at:at + size])
                    at += size

    def _reference_for(self, path, lengths):
        """The RefSeq kept for this file and these lengths, or None."""
        kept = self._reference
        key = (path, tuple(sorted(lengths.items())))
        return kept[1] if kept is not None and kept[0] == key and kept[1].handle else None

    def reference_on(self, args, hip, lengths, acc_index):
        """The reference of the run on the device (Hip.refseq_from_file): parsed once, and again only where an input file's lengths
        differ from those it was parsed for."""
        path = self.reference(args)
        ref = self._reference_for(path, lengths)
        if ref is None:
            if self._reference is not None:
                self._reference[1].free()
                self._reference = None
            names = [None] * len(acc_index)
            for a, i in acc_index.items():
                names[i] = a
            index = hip.acc_index(names)
            try:
                ref = hip.refseq_from_file(path, index, lengths_array(lengths, acc_index))
            except _hip.HipError as e:
                if e.code != _hip.ERR_NOMEM:
                    raise
                sys.exit('Error: --ani and --vcf keep the reference FASTA and one byte per reference base on the GPU: %s' % e)
            finally:
                index.free()
            self._reference = ((path, tuple(sorted(lengths.items()))), ref)
        return ref

    def diff_from(self, args, lengths, dev, acc_index, acc2info, aln, call, unpiled):
        """--ani / --vcf from the open accumulator -> refdiff.RefDiff."""
        p = self.params(args)
        ref = self.reference_on(args, dev.hip, lengths, acc_index)
        comp, con, pop, other, sites = dev.diff(ref, *p)
        loaded = ref.loaded()
        emitted = np.bincount(sites['acc'], minlength=len(acc_index)) if len(sites) else np.zeros(len(acc_index), dtype=np.int64)
        per = {a: [int(aln[i]), int(call[i]), int(comp[i]), int(con[i]), int(pop[i]), int(other[i]), int(emitted[i])]
               for a, i in acc_index.items() if aln[i] and loaded[i]}
        no_reference = sum(1 for a, i in acc_index.items() if aln[i] and not loaded[i])
        names = {i: a for a, i in acc_index.items()}
        order = {a: k for k, a in enumerate(acc2info)}  # (the device orders by accession row, the files by db_info's order)
        rows = sorted(((names[int(s['acc'])], int(s['pos0']), tuple(int(x) for x in s['n']), int(s['ref'])) for s in sites),
                      key=lambda s: (order[s[0]], s[1]))
        return refdiff.RefDiff(lengths, per, rows, unpiled, no_reference)

    def append_diff(self, args, source, diff, acc2info, taxid2info):
        p = self.params(args)
        if _flag(args, 'ani'):
            refdiff.write_ani(args.ani, p, refdiff.rows(diff, acc2info, taxid2info), diff.unpiled, diff.no_reference,
                              source=source_label(args, source), append=True)
        if _flag(args, 'vcf'):
            refdiff.write_vcf(args.vcf, diff, self.reference(args), acc2info, p, reads_mode(args) == 'unique')

    def append(self, args, source, var, acc2info, taxid2info):
        p, source = self.params(args), source_label(args, source)
        if _flag(args, 'variants'):
            variants.write_variants(args.variants, p, variants.rows(var, acc2info, taxid2info), var.unpiled, source=source, append=True)
        if _flag(args, 'variant_sites'):
            variants.write_sites(args.variant_sites, p, var.sites, source=source, append=True)

    def append_from_definition(self, args, path, lines, acc2info, taxid2info):
        if not any(_flag(args, f) for f in self.riders):
            self.append(args, path, variants.variants(lines, acc2info, args.pct_id, self.params(args)), acc2info, taxid2info)
            return
        # (one pass over the lines, which come as an iterator: variants.variants, consensus.consensus and refdiff.refdiff are these
        # over them)
        p, iupac, order = self.params(args), self.iupac(args), list(acc2info)
        n, aln, unpiled, lengths = variants.counts_of_lines(lines, acc2info, args.pct_id)
        if _Family.wanted(self, args):
            self.append(args, path, variants.summarise(n, aln, unpiled, lengths, order, p), acc2info, taxid2info)
        if _flag(args, 'consensus'):
            recs = consensus.records_of(n, aln, unpiled, lengths, order, acc2info, p, iupac, getattr(args, 'consensus_min_called', 0.0))
            consensus.write_consensus(args.consensus, recs, True, p, iupac, reads_mode(args) == 'unique', source_label(args, path))
        if self.diffed(args):
            acc_index = {a: i for i, a in enumerate(order)}
            parsed = refseq.parse(refseq.read_bytes(self.reference(args)), acc_index, [lengths[a] for a in order])
            ref = refdiff.ref_by_accession(parsed, acc_index)
            self.append_diff(args, path, refdiff.compare(n, aln, unpiled, lengths, order, ref, p), acc2info, taxid2info)


ASSIGNMENTS, COVERAGE, DEPTH, IDENTITY, VARIANTS = _Assignments(), _Coverage(), _Depth(), _Identity(), _Variants()
FAMILIES = (COVERAGE, DEPTH, IDENTITY, VARIANTS)  # (the order of every open, add and close)


def aligner_is_device(args):
    """--aligner device (callers build Namespaces without it: minimap2)."""
    return getattr(args, 'aligner', 'minimap2') == 'device'


def align_params(args):
    """--align_* -> align.Params; ValueError names the first value out of its range."""
    from . import align
    return align.params(getattr(args, 'align_k', align.K), getattr(args, 'align_w', align.W), getattr(args, 'align_max_occ', align.MAX_OCC),
                        getattr(args, 'align_min_score', align.MIN_SCORE), getattr(args, 'align_mismatch', align.MISMATCH),
                        getattr(args, 'align_secondary', align.MAX_SECONDARY), getattr(args, 'align_secondary_pct', align.SEC_PCT))


def align_gap_params(args):
    """--align_band, --align_gap_open, --align_gap_extend -> align.GapParams; ValueError names the first value out of its range."""
    from . import align
    return align.gap_params(getattr(args, 'align_band', align.BAND), getattr(args, 'align_gap_open', align.GAP_OPEN),
                            getattr(args, 'align_gap_extend', align.GAP_EXTEND))


def align_pair_params(args):
    """--align_pairs, --align_max_insert, --align_rescue -> align.PairParams; ValueError names the first value out of its range."""
    from . import align
    return align.pair_params(getattr(args, 'align_pairs', 'none'), getattr(args, 'align_max_insert', align.MAX_INSERT),
                             getattr(args, 'align_rescue', align.RESCUE))


def check_aligner_flags(args):
    """--aligner device: what it cannot be combined with, and the ranges of its parameters.  Alignment files (SAM / BAM / PAF, by
    --input_type or the first file's name, as map_main decides) are not aligned: the flag is a no-op there."""
    if getattr(args, 'align_pairs', 'none') != 'none' and not aligner_is_device(args):
        sys.exit('Error: --align_pairs pairs the reads in the aligner on the GPU: it needs --aligner device.')
    if not aligner_is_device(args):
        return
    files = getattr(args, 'infiles', ())
    if getattr(args, 'input_type', 'AUTO') == 'sam' or (files and files[0].endswith(('sam', 'paf', 'bam')) and not hasattr(args, 'reads')):
        return
    if ASSIGNMENTS.wanted(args):
        sys.exit('Error: --aligner device keeps no read names: --read_assignments needs --aligner minimap2 or an alignment file.')
    if getattr(args, 'collate', 'never') != 'never':
        sys.exit('Error: --aligner device writes a read\'s alignments next to each other: --collate must stay "never".')
    try:
        align_params(args)
        align_gap_params(args)
        pairs = align_pair_params(args)
    except ValueError as e:
        sys.exit('Error: %s' % e)
    if pairs.interleaved and hasattr(args, 'reads') and os.path.isfile(args.reads):
        from . import bam
        if bam.is_bam(args.reads):
            sys.exit('Error: --align_pairs interleaved pairs by position, and the mates of a BAM of reads are not next to each other '
                     'in its FASTQ rendering: give an interleaved FASTQ / FASTA file.')


def check_flags(args):
    """What map_main and metalign.main refuse before a process group, the library or a GPU is touched."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    check_aligner_flags(args)
    paf = getattr(args, 'paf_input', False) or any(f.endswith('.paf') for f in getattr(args, 'infiles', ()))
    for fam in (ASSIGNMENTS,) + FAMILIES:
        if not fam.wanted(args):
            continue
        if world > 1:
            sys.exit(fam.refusal(args, 'world'))
        if paf and fam.refusal(args, 'paf'):
            sys.exit(fam.refusal(args, 'paf'))
    VARIANTS.check_reference(args)
    if int(getattr(args, 'depth_window_size', 1000)) < 1:
        sys.exit('Error: --depth_window_size must be at least 1.')
    try:
        VARIANTS.params(args)
        VARIANTS.min_called(args)
    except ValueError as e:
        sys.exit('Error: %s' % e)
    if reads_mode(args) == 'unique' and not any(fam.wanted(args) for fam in FAMILIES):
        sys.exit('Error: --side_reads unique needs one of --coverage, --depth, --depth_windows, --identity.')


def write_headers(args):
    """Rank 0, once: the header of every output that was asked for; every input file appends to them."""
    for fam in (ASSIGNMENTS,) + FAMILIES:
        if fam.wanted(args):
            fam.write_header(args)
            if fam in FAMILIES and reads_mode(args) == 'unique':
                for path in fam.paths(args):
                    with open(path, 'a') as out:
                        out.write(side_reads.HEADER_LINE)


class SideOutputs:
    """The families wanted for one input file.  source: the name its blocks are written under.  header: the file's header lines,
    whose @SQ lines give the lengths (None: the caller takes them from the stream)."""

    def __init__(self, args, families, source, header=None):
        self.args, self.source, self.header = args, source, header
        self.families = tuple(f for f in FAMILIES if f in families)
        self.placed = any(f.side == 'places' for f in self.families)
        self.edited = any(f.side == 'edits' for f in self.families)
        self.based = any(f.side == 'bases' for f in self.families)
        self.sized = self.placed or self.based  # (the families that need the accessions' lengths)
        self.reads = reads_mode(args)
        self.unique = bool(self.families) and self.reads == 'unique'
        self._open = []  # (family, accumulator) of what is open
        self._lengths = self._acc_index = None

    @classmethod
    def of(cls, args, source, header=None, enabled=True):
        """What args asks for (enabled=False: nothing).  header: a callable, called where an output needs the lengths."""
        sides = cls(args, [f for f in FAMILIES if enabled and f.wanted(args)], source)
        if header is not None and sides.sized:
            sides.header = header()
        return sides

    def __bool__(self):
        return bool(self.families)

    def need_bytes(self, lengths, nacc, nrec):
        """What the accumulators and the side arrays of nrec records hold on the device."""
        # 8 B of place per record (and as much again where a collation permutes them), once for coverage and depth
        need = 16 * nrec if self.placed else 0
        if self.unique:
            need += 32 * nrec  # the masked copy of the records, and at most 16 B of verdict words per record
        return need + sum(f.device_bytes(self.args, lengths, nacc, nrec) for f in self.families)

    def open(self, hip, lengths, acc_index):
        self._lengths, self._acc_index = lengths, acc_index
        try:
            for fam in self.families:
                self._open.append((fam, fam.open(self.args, hip, lengths, acc_index)))
        except BaseException:
            self.free()
            raise

    def on_verdicts(self, hip, batch, pct_id):
        """The on_verdicts hook of Hip.profile_assign_dev_records over `batch` under --side_reads unique: the records, masked by their
        reads' verdicts, go to the accumulators beside the batch's side arrays, from inside stage C.  None where the accumulators are
        fed before stage C (add_batch)."""
        if not self.unique:
            return None

        def feed(d_recs, n, d_words, nreads, d_ref2tax, nref):
            if n:  # (as add_batch: an empty stream adds nothing)
                self.add_unique_ptrs(hip, d_recs, batch.places_ptr if self.placed else None, batch.edits_ptr if self.edited else None, n,
                                     pct_id, d_words, nreads, d_ref2tax, nref, (batch.bases_ptr, batch.pool_ptr) if self.based else None)
        return feed

    def add_batch(self, batch, pct_id):
        """A batch (SamBatch, UploadedBatch) that carries every side array the families read."""
        try:
            for _, dev in self._open:
                dev.add_batch(batch, pct_id)
        except BaseException:
            self.free()
            raise

    def add_ptrs(self, d_recs, d_places, d_edits, n, pct_id, d_bases=None):
        """n records and their side arrays at device pointers (asynchronous, as the accumulators' add_ptr).  d_bases: the pair
        (entries, pool)."""
        side = {'places': d_places, 'edits': d_edits, 'bases': d_bases}
        try:
            for fam, dev in self._open:
                dev.add_ptr(d_recs, side[fam.side], n, pct_id)
        except BaseException:
            self.free()
            raise

    def add_unique_ptrs(self, hip, d_recs, d_places, d_edits, n, pct_id, d_words, nreads, d_ref2tax, nref, d_bases=None):
        """add_ptrs under --side_reads unique, from inside stage C: the records go through mg_records_mask_unique_dev into a copy,
        which is what the accumulators read.  Returns with the work done: the copy is freed on every way out."""
        copy = None
        try:
            copy = hip.empty(16 * max(int(n), 1), np.uint8)
            hip.records_mask_unique(d_recs, n, d_words, nreads, d_ref2tax, nref, copy.ptr)
            self.add_ptrs(copy.ptr, d_places, d_edits, n, pct_id, d_bases)  # (the masked records beside the untouched entries)
            hip.sync()
        except BaseException:
            self.free()
            raise
        finally:
            if copy is not None:
                copy.free()

    def close(self, acc2info, taxid2info):
        """Every accumulator -> its block, appended to its file."""
        try:
            while self._open:
                fam, dev = self._open.pop(0)  # (the family's close frees it)
                fam.close(self.args, self.source, self._lengths, dev, self._acc_index, acc2info, taxid2info)
        finally:
            self.free()

    def free(self):
        """Whatever is still open, once."""
        while self._open:
            self._open.pop()[1].free()

    def append_from_definition(self, path, lines, acc2info, taxid2info):
        """The host definitions over a line stream (lines(): a fresh iterator): the outputs do not depend on the lines' order."""
        for fam in self.families:
            fam.append_from_definition(self.args, path, lines(), acc2info, taxid2info)
