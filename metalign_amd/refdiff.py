"""The pileup compared with the reference it was aligned to (--ani, --vcf): the definition, on the host.

--variant_sites lists where the reads disagree with each other; a sample that carries one strain 2 % away from the database genome
has almost no such site.  This compares variants.py's counts with the reference base (refseq.py): substitutions against the
reference, the consensus and population ANI of every detected accession to its database entry (inStrain's conANI and popANI) and a
VCF.  Which lines count, how they are piled, the counts, the thresholds (D, C, F) = variants.params and the site rule
variants.site_of are variants.py's: used, not restated.  On top, for a site with counts n4 and reference code r, on an accession
with a piled alignment and a loaded reference (diff_of):

  COMPARED    the site is callable (d >= D) and r < 4;  `ref_other`: callable and r == 4.
  present     {major} and the variant alleles.
  con_sub     compared and major != r;  pop_sub: compared and r not in present.
  EMITTED     compared and present - {r} is not empty: a con_sub or a polymorphic site.

  Per accession.  compared, con_subs, pop_subs, ref_other, emitted; a genome sums its accessions.  conANI = 1 - con_subs / compared,
      popANI = 1 - pop_subs / compared: exact (Fractions) until they are printed, 0 where compared is 0.
  Rows.  An S row per accession with a piled alignment AND a loaded reference in db_info order, then a G row per taxid that has one,
      its length the sum over all its accessions (the convention of variants.rows).  The block ends with `#unpiled\\tN` and
      `#no_reference\\tN`: the accessions with a piled alignment and no loaded reference, which get no S row.
  VCF (format_vcf).  VCFv4.2; one line per emitted site in (db_info order, position) order: REF the reference letter in upper case,
      ALT the members of present - {r}, the highest count first, ties to the lowest code; DP = d, AD = n_ref and the ALTs' counts,
      AF = n_alt / d as %.6f.

All of it is integer, so the device (mg_variants.hip: k_var_diff; mg_variants_core.h: diff_of) is held to it exactly.
"""
from collections import namedtuple
from fractions import Fraction

from . import variants

HEADER = '#kind\tid\ttaxid\tlength\talignments\tcallable_sites\tcompared_sites\tcon_subs\tpop_subs\tref_other\tconANI\tpopANI\n'
VCF_COLUMNS = '#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n'

# per {accession: [alignments, callable, compared, con_subs, pop_subs, ref_other, emitted]} (a piled alignment and a loaded
# reference); sites [(accession, pos0, (nA, nC, nG, nT), r)] — the emitted ones, in db_info order, then by position
RefDiff = namedtuple('RefDiff', 'lengths per sites unpiled no_reference')
Diff = namedtuple('Diff', 'compared ref_other con_sub pop_sub emitted alts')


def diff_of(n4, r, p):
    """One site's four counts and its reference code -> Diff; alts: present - {r} in the order of ALT."""
    ok, major, var, _, _ = variants.site_of(n4, p)
    if not ok:
        return Diff(False, False, False, False, False, [])
    if r >= 4:
        return Diff(False, True, False, False, False, [])
    present = [major] + var
    alts = sorted((a for a in present if a != r), key=lambda a: (-n4[a], a))
    return Diff(True, False, major != r, r not in present, bool(alts), alts)


def compare(n, aln, unpiled, lengths, order, ref, p):
    """accumulate()'s three and ref {accession: its codes (bytes), the loaded ones} -> RefDiff.  order: db_info's."""
    per, sites, no_ref = {}, [], 0
    called = variants.summarise(n, aln, unpiled, lengths, order, p).per
    for acc in order:
        if not aln.get(acc):
            continue
        codes = ref.get(acc)
        if codes is None:
            no_ref += 1
            continue
        st = [aln[acc], called[acc][1], 0, 0, 0, 0, 0]
        for pos in sorted(n.get(acc, {})):
            n4 = n[acc][pos]
            d = diff_of(n4, codes[pos], p)
            st[2] += d.compared
            st[3] += d.con_sub
            st[4] += d.pop_sub
            st[5] += d.ref_other
            if d.emitted:
                st[6] += 1
                sites.append((acc, pos, tuple(n4), codes[pos]))
        per[acc] = st
    return RefDiff(lengths, per, sites, unpiled, no_ref)


def ref_by_accession(parsed, acc_index):
    """refseq.parse's result -> {accession: codes} of the loaded rows."""
    return {a: parsed.codes[i] for a, i in acc_index.items() if parsed.loaded[i]}


def refdiff(lines, acc2info, pct_id, ref, p=None):
    """SAM lines (str or bytes; the header among them) and ref {accession: codes} -> RefDiff."""
    n, aln, unpiled, lengths = variants.counts_of_lines(lines, acc2info, pct_id)
    return compare(n, aln, unpiled, lengths, list(acc2info), ref, p or variants.params())


def rows(diff, acc2info, taxid2info):
    """-> [(kind, id, taxid, length, alignments, callable, compared, con_subs, pop_subs, ref_other)], S rows then G rows."""
    out, by_tax = [], {}
    for acc, info in acc2info.items():
        g = by_tax.setdefault(info[1], [0, 0, 0, 0, 0, 0, 0])
        g[0] += diff.lengths[acc]
        st = diff.per.get(acc)
        if st is None or st[0] < 1:
            continue
        out.append(('S', acc, info[1], diff.lengths[acc]) + tuple(st[:6]))
        for i in range(6):
            g[1 + i] += st[i]
    for taxid in taxid2info:
        g = by_tax.get(taxid)
        if g is not None and g[1] >= 1:
            out.append(('G', taxid, taxid) + tuple(g))
    return out


def ani(compared, con_subs, pop_subs):
    """-> (conANI, popANI), exact; 0 where nothing was compared."""
    if not compared:
        return Fraction(0), Fraction(0)
    return 1 - Fraction(con_subs, compared), 1 - Fraction(pop_subs, compared)


def format_row(row):
    kind, ident, taxid, length, aln, call, comp, con, pop, other = row
    con_ani, pop_ani = ani(comp, con, pop)
    return '%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f\t%.6f\n' % (kind, ident, taxid, length, aln, call, comp, con, pop, other,
                                                                       float(con_ani), float(pop_ani))


def format_block(block_rows, unpiled, no_reference, source=None):
    """One input file's block: `#file\\t<source>` (several input files only), its rows, `#unpiled\\t<n>`, `#no_reference\\t<n>`."""
    head = '#file\t%s\n' % source if source is not None else ''
    return head + ''.join(format_row(r) for r in block_rows) + '#unpiled\t%d\n#no_reference\t%d\n' % (unpiled, no_reference)


def write_ani(path, p=None, block_rows=None, unpiled=0, no_reference=0, source=None, append=False):
    """TSV: the column header and the line that names D, C and F (a new file only), then — unless block_rows is None — one block."""
    with open(path, 'a' if append else 'w') as out:
        if not append:
            out.write(HEADER + variants.params_line(p or variants.params()))
        if block_rows is not None:
            out.write(format_block(block_rows, unpiled, no_reference, source))


def vcf_header(reference, contigs, p, unique=False):
    """contigs: [(accession, length)] of the accessions with an S row, in db_info order."""
    return ('##fileformat=VCFv4.2\n##source=metalign_amd\n##reference=%s\n' % reference
            + ''.join('##contig=<ID=%s,length=%d>\n' % c for c in contigs)
            + '##INFO=<ID=DP,Number=1,Type=Integer,Description="Reads with A, C, G or T at the site">\n'
            + '##INFO=<ID=AD,Number=R,Type=Integer,Description="Reads per allele, the reference allele first">\n'
            + '##INFO=<ID=AF,Number=A,Type=Float,Description="Share of DP per alternative allele">\n'
            + '##metalign_variants=min_depth=%d,min_count=%d,min_freq_permille=%d,reads=%s\n' % (tuple(p) + ('unique' if unique else 'all',))
            + VCF_COLUMNS)


def format_vcf_site(site, p):
    acc, pos0, n4, r = site
    alts = diff_of(n4, r, p).alts
    d = sum(n4)
    return '%s\t%d\t.\t%s\t%s\t.\tPASS\tDP=%d;AD=%s;AF=%s\n' % (
        acc, pos0 + 1, variants.LETTERS[r], ','.join(variants.LETTERS[a] for a in alts), d,
        ','.join('%d' % n4[a] for a in [r] + alts), ','.join('%.6f' % (n4[a] / d) for a in alts))


def format_vcf(diff, reference, acc2info, p, unique=False):
    """-> str: the whole VCF of one input file."""
    contigs = [(a, diff.lengths[a]) for a in acc2info if a in diff.per]
    return vcf_header(reference, contigs, p, unique) + ''.join(format_vcf_site(s, p) for s in diff.sites)


def write_vcf(path, diff, reference, acc2info, p=None, unique=False):
    with open(path, 'w') as out:
        out.write(format_vcf(diff, reference, acc2info, p or variants.params(), unique))
