"""Command-line surface shared by the three entry points.

The flag names, defaults, types, choices and sentinels ('AUTO', 'NONE', 'AUTO/') are the reference's
(/root/reference/scripts/metalign.py:8-40, select_db.py:5-24, map_and_profile.py:20-45) so that existing
invocations keep working; tests/test_select_and_cli.py checks them against a fixture dumped from the reference's
own parsers.  They are declared once here, as data, and each tool picks the subset it accepts.
"""
import argparse
import sys

# name -> (argparse kwargs).  Store-true switches carry action='store_true'.
_OPTIONS = {
    'cmash_results': dict(default='NONE', help='Existing containment CSV to reuse (skips the GPU pre-filter).'),
    'cutoff': dict(type=float, default=0.01, help='Keep organisms whose containment index is at least this (default 0.01).'),
    'db': None,  # differs per tool, see below
    'db_dir': dict(default='AUTO', help='Directory holding one FASTA(.gz) per organism of the full database.'),
    'dbinfo': dict(default='AUTO', help='db_info file to profile against (default: data/db_info.txt).'),
    'dbinfo_in': dict(default='AUTO', help='db_info of the full database (default: data/db_info.txt).'),
    'dbinfo_out': dict(default='AUTO', help='Where the subset db_info goes (default: temp_dir/subset_db_info.txt).'),
    'input_type': None,  # differs per tool
    'keep_temp_files': dict(action='store_true', help='Leave the temporary directory in place.'),
    'length_normalize': dict(action='store_true', help='Divide base counts by genome length.'),
    'low_mem': dict(action='store_true', help='Low-memory handling of multimapped reads (inexact).'),
    'min_abundance': dict(type=float, default=10**-4, help='Do not report taxa below this abundance (default 1e-4).'),
    'no_quantify_unmapped': dict(action='store_true', help='Ignore unmapped reads when computing abundances.'),
    'output': dict(default='abundances.tsv', help='CAMI profile to write (default abundances.tsv).'),
    'pct_id': dict(type=float, default=0.5, help='Minimum matched fraction of an alignment for it to count (default 0.5).'),
    'precise': dict(action='store_true', help='Precise mode: read_cutoff 100, min_abundance 0.1.'),
    'rank_renormalize': dict(action='store_true', help='Rescale every rank to the mapped percentage.'),
    'read_cutoff': dict(type=int, default=1, help='An organism needs MORE than this many unique reads (default 1).'),
    'sampleID': dict(default='NONE', help='Sample ID written to the profile header (default: input file names).'),
    'sensitive': dict(action='store_true', help='Sensitive mode: containment cutoff 0.'),
    'strain_level': dict(action='store_true', help='Keep every strain above the cutoff instead of one per species.'),
    'temp_dir': dict(default='AUTO/', help='Directory for intermediate files (default: a fresh one under data/).'),
    'threads': dict(type=int, default=4, help='Threads handed to the aligner (default 4).'),
    'verbose': dict(action='store_true', help='Progress messages.'),
    # build-only additions; defaults reproduce the reference behaviour
    'sketch_table': dict(default='AUTO', help='Genome sketch table directory (default: data/sketch_table).'),
    'min_count': dict(type=int, default=2, help='A read k-mer must occur this often to count (kmc -ci, default 2).'),
    'sketch_size': dict(type=int, default=0, help='Read sketch size per k; 0 keeps every hash up to the table maximum.'),
    'kmer_match': dict(default='identity', choices=['identity', 'identity_only', 'hash'],
                       help='A reference-pipeline sketch table: a read k-mer meets a sketched one by what it IS, as kmc and kmc_tools '
                            'intersect compare k-mers (default where it is the faster way: a table that stores its k-mers, the largest k '
                            'from 25 to 64; "hash" otherwise), wherever that can run at all (identity_only: the largest k from 15 to 64), or '
                            'by its MurmurHash3 value.'),
    'collate': dict(default='never', choices=['never', 'auto', 'always'],
                    help='Regroup the alignments of a SAM / BAM file by read before profiling, on the GPU: "auto" when the @HD line '
                         'says SO:coordinate, "always", or "never" (default: a read\'s alignments are expected next to each other). '
                         'An aligner\'s own output is never regrouped.'),
    'read_assignments': dict(default='NONE', help='Also write every read\'s verdict here, one TSV line per read in file order: '
                             'read, class (U unique / M multimapped / A ambiguous / N not counted: the last read), taxids, hit bases '
                             '(metalign_amd/assignments.py is the definition). One process only.'),
    'coverage': dict(default='NONE', help='Also write breadth and depth of coverage here (TSV): per accession (S rows) and per '
                     'genome (G rows) the placed alignments, aligned bases, covered bases, breadth, mean depth and the breadth that '
                     'depth predicts, from the alignments stage C keeps (metalign_amd/coverage.py is the definition). SAM / BAM '
                     'input, one process only.'),
    'identity': dict(default='NONE', help='Also write alignment identity here (TSV): per accession (S rows) and per genome (G rows) '
                     'the scored alignments, their aligned columns and summed edit distance (NM:i:), the identity those give, the '
                     'median and 10th percentile of per-alignment identity and the alignments at 90, 95, 97 and 99 %% or more '
                     '(metalign_amd/identity.py is the definition). SAM / BAM input, one process only.'),
    'depth': dict(default='NONE', help='Also write the distribution of per-base depth here (TSV): per accession (S rows) and per '
                  'genome (G rows) the mean, median, 5-95 %% trimmed mean, variance and maximum of the depth (clamped at 4095) and the '
                  'bases at 1x, 5x, 10x and 30x or more (metalign_amd/depth.py is the definition). SAM / BAM input, one process only.'),
    'depth_windows': dict(default='NONE', help='Also write the depth along every accession here (TSV): per window of '
                          '--depth_window_size bases that an alignment touches, the mean depth and the covered bases.'),
    'depth_window_size': dict(type=int, default=1000, help='The width of the windows of --depth_windows (default 1000; 1 gives the '
                              'depth of every base).'),
    'variants': dict(default='NONE', help='Also write per-genome strain diversity here (TSV): per accession (S rows) and per genome '
                     '(G rows) the piled alignments, the callable and the polymorphic sites, the read pairs compared and the '
                     'discordant ones, nucleotide diversity pi and polymorphic sites per kb, from the read bases of the alignments '
                     'stage C keeps (metalign_amd/variants.py is the definition). SAM / BAM input, one process only.'),
    'variant_sites': dict(default='NONE', help='Also write every polymorphic site here (TSV): accession, position, depth, the '
                          'reads\' A, C, G and T, the major allele and the variant alleles.'),
    'variant_min_depth': dict(type=int, default=5, help='A site is callable from this many A / C / G / T reads on (default 5, at '
                              'least 2).'),
    'variant_min_count': dict(type=int, default=2, help='A variant allele has at least this many reads (default 2, at least 1).'),
    'variant_min_freq': dict(type=float, default=0.05, help='... and at least this share of the site\'s depth (default 0.05, within '
                             '0 to 0.5; compared in parts per thousand).'),
    'consensus': dict(default='NONE', help='Also write the consensus sequence of every accession with a piled alignment here '
                      '(FASTA, lines of 60): per reference base the major allele of the reads, N below --variant_min_depth, from the '
                      'allele counts --variants keeps (metalign_amd/consensus.py is the definition). SAM / BAM input, one process '
                      'only.'),
    'consensus_ambiguity': dict(default='major', choices=['major', 'iupac'],
                                help='A polymorphic site of --consensus: "major" writes its major allele (default), "iupac" the IUPAC '
                                     'code of the major and the variant alleles (--variant_min_count, --variant_min_freq).'),
    'consensus_min_called': dict(type=float, default=0.0, help='Write an accession to --consensus only when at least this share of '
                                 'its bases is callable (default 0.0, within 0 to 1; compared in parts per thousand).'),
    'ani': dict(default='NONE', help='Also write the consensus and population ANI of every detected accession to its reference '
                'sequence here (TSV): per accession (S rows) and per genome (G rows) the callable sites compared with a reference '
                'A / C / G / T, the substitutions of the consensus (the major allele differs) and of the population (the reference '
                'base is no allele of the sample), conANI and popANI (metalign_amd/refdiff.py is the definition). Needs the '
                'reference FASTA (--reference). SAM / BAM input, one process only.'),
    'vcf': dict(default='NONE', help='Also write every site where the sample differs from the reference here (VCFv4.2): REF, the '
                'alleles of the sample that are not REF as ALT, DP, AD and AF. One input file only. Needs the reference FASTA '
                '(--reference).'),
    'reference': dict(default='AUTO', help='The FASTA (optionally .gz) the reads were aligned to, for --ani and --vcf (default: '
                      'the database FASTA the aligner gets, --db).'),
    'side_reads': dict(default='all', choices=['all', 'unique'],
                       help='Which alignments --coverage, --depth, --depth_windows and --identity count: "all" that pass --pct_id (the '
                            'default), or "unique": only those of reads the profile assigned uniquely, on an accession of the taxon '
                            'the read was counted for (metalign_amd/side_reads.py is the definition).'),
    'multimap_iterations': dict(type=int, default=1, help='Iterate the reassignment of multimapped reads up to this many times: every '
                                'iteration shares them in proportion to the bases the one before gave (metalign_amd/multimap.py is '
                                'the definition). Default 1: the single step, in proportion to uniquely mapped bases.'),
    'multimap_tol': dict(type=float, default=1e-8, help='Stop iterating once no genome\'s bases change by more than this fraction '
                         '(default 1e-8, a tenth of the last digit the profile prints); 0 runs all --multimap_iterations.'),
    'aligner': dict(default='minimap2', choices=['minimap2', 'device'],
                    help='What aligns a reads file: "minimap2" (default: the external program, started as the reference starts it) or '
                         '"device": the seed-and-extend aligner on the GPU (metalign_amd/align.py is the definition), which needs no '
                         'minimap2 installed and ignores --threads. It is ungapped unless --align_band is given, single-end unless --align_pairs is given, gives no MAPQ, keeps no read names '
                         '(no --read_assignments) and runs on one GPU; it is not minimap2 and does not reproduce its alignments. '
                         'No effect on SAM / BAM / PAF input.'),
    'align_k': dict(type=int, default=15, help='--aligner device: the k-mer length of the seeds (default 15; odd, 11 to 31).'),
    'align_w': dict(type=int, default=5, help='--aligner device: the minimizer window, in k-mers (default 5; 1 to 32).'),
    'align_max_occ': dict(type=int, default=64, help='--aligner device: a minimizer that occurs more often than this in the '
                          'reference seeds nothing (default 64).'),
    'align_min_score': dict(type=int, default=30, help='--aligner device: an alignment scores at least this (default 30; a match '
                            'adds 1).'),
    'align_mismatch': dict(type=int, default=4, help='--aligner device: what a mismatch subtracts (default 4).'),
    'align_secondary': dict(type=int, default=5, help='--aligner device: at most this many secondary alignments per read '
                            '(default 5; 0 to 15).'),
    'align_secondary_pct': dict(type=int, default=80, help='--aligner device: a secondary alignment has at least this percentage '
                                'of the primary\'s score (default 80).'),
    'align_band': dict(type=int, default=0, help='--aligner device: gapped extension. 0 (default): none, the aligner is ungapped. '
                       'B in 1 to 31: an alignment that does not cover its whole read is redone with affine gaps within B diagonals '
                       'of its seed\'s, which finds insertions and deletions of up to B bases (8 is a good value for short reads).'),
    'align_gap_open': dict(type=int, default=6, help='--align_band: what opening a gap subtracts (default 6; 0 to 64). A gap of g '
                           'bases costs --align_gap_open + g * --align_gap_extend.'),
    'align_gap_extend': dict(type=int, default=1, help='--align_band: what each base of a gap subtracts (default 1; 1 to 64).'),
    'align_pairs': dict(default='none', choices=['none', 'interleaved'],
                        help='--aligner device: paired-end reads. "none" (default): every read is a read of its own. "interleaved": '
                             'reads 2i and 2i + 1 of the file are mates 1 and 2 of pair i; the mates rescue each other, the records are '
                             'chosen per pair and carry the pair\'s FLAG bits. Pairing is BY POSITION: the aligner keeps no read names '
                             'and compares none. An odd number of reads is an error. Not for a BAM of reads.'),
    'align_max_insert': dict(type=int, default=1000, help='--align_pairs: the largest outer distance of a proper pair, in bases '
                             '(default 1000; 1 to 8192).'),
    'align_rescue': dict(type=int, default=2, help='--align_pairs: how many of a mate\'s best alignments may each rescue the other mate '
                         'within --align_max_insert of them (default 2; 0 to 8, 0: no rescue).'),
    'device_multimap': dict(action='store_true', help='Resolve multimapped reads on the GPU (their lists never leave '
                            'the device; abundances equal the default path to ~1e-15 relative, not byte for byte).'),
}

_READ_TYPES = ['fastq', 'fasta', 'AUTO']

_TOOLS = {
    'metalign': dict(
        description='Runs full metalign pipeline on input reads file(s).',
        positionals=[('reads', dict(help='Reads file (FASTA / FASTQ, optionally .gz, or a BAM of reads; a paired BAM is aligned '
                                          'single-end, as one reads file is).')),
                     ('data', dict(help='data/ directory (db_info.txt, organism_files/, sketch_table/).'))],
        options=['cutoff', 'db_dir', 'dbinfo_in', 'keep_temp_files', ('input_type', _READ_TYPES), 'length_normalize',
                 'low_mem', 'min_abundance', 'no_quantify_unmapped', 'output', 'pct_id', 'precise', 'rank_renormalize',
                 'read_cutoff', 'sampleID', 'sensitive', 'strain_level', 'temp_dir', 'threads', 'verbose',
                 'sketch_table', 'min_count', 'sketch_size', 'kmer_match', 'device_multimap', 'collate', 'read_assignments', 'coverage',
                 'multimap_iterations', 'multimap_tol', 'depth', 'depth_windows', 'depth_window_size', 'identity', 'side_reads',
                 'variants', 'variant_sites', 'variant_min_depth', 'variant_min_count', 'variant_min_freq',
                 'consensus', 'consensus_ambiguity', 'consensus_min_called', 'ani', 'vcf', 'reference',
                 'aligner', 'align_k', 'align_w', 'align_max_occ', 'align_min_score', 'align_mismatch', 'align_secondary',
                 'align_secondary_pct', 'align_band', 'align_gap_open', 'align_gap_extend', 'align_pairs', 'align_max_insert',
                 'align_rescue']),
    'select_db': dict(
        description='Run CMash and select a subset of the whole database to align to.',
        positionals=[('reads', dict(help='Reads file (FASTA / FASTQ, optionally .gz, or a BAM of reads).')),
                     ('data', dict(help='data/ directory (db_info.txt, organism_files/, sketch_table/).'))],
        options=['cmash_results', 'cutoff', ('db', 'AUTO', 'Subset database FASTA to write (default: temp_dir/cmashed_db.fna).'),
                 'db_dir', 'dbinfo_in', 'dbinfo_out', ('input_type', _READ_TYPES), 'keep_temp_files', 'strain_level',
                 'temp_dir', 'threads', 'sketch_table', 'min_count', 'sketch_size', 'kmer_match']),
    'map_and_profile': dict(
        description='Compute abundance estimations for species in a sample.',
        positionals=[('infiles', dict(nargs='+', help='SAM file(s), or reads file(s) to align (--aligner: with minimap2, or on the GPU).')),
                     ('data', dict(help='data/ directory.'))],
        options=[('db', 'NONE', 'Database FASTA from select_db (needed unless the inputs are SAM files).'), 'dbinfo',
                 ('input_type', ['fastq', 'fasta', 'sam', 'AUTO']), 'length_normalize', 'low_mem', 'min_abundance',
                 'rank_renormalize', 'output', 'pct_id', 'no_quantify_unmapped', 'read_cutoff', 'sampleID', 'threads',
                 'verbose', 'device_multimap', 'collate', 'read_assignments', 'coverage',
                 'multimap_iterations', 'multimap_tol', 'depth', 'depth_windows', 'depth_window_size', 'identity', 'side_reads',
                 'variants', 'variant_sites', 'variant_min_depth', 'variant_min_count', 'variant_min_freq',
                 'consensus', 'consensus_ambiguity', 'consensus_min_called', 'ani', 'vcf', 'reference',
                 'aligner', 'align_k', 'align_w', 'align_max_occ', 'align_min_score', 'align_mismatch', 'align_secondary',
                 'align_secondary_pct', 'align_band', 'align_gap_open', 'align_gap_extend', 'align_pairs', 'align_max_insert',
                 'align_rescue']),
}


def parser_for(tool):
    spec = _TOOLS[tool]
    p = argparse.ArgumentParser(description=spec['description'])
    for name, kw in spec['positionals']:
        p.add_argument(name, **kw)
    for opt in spec['options']:
        if isinstance(opt, tuple) and opt[0] == 'input_type':
            p.add_argument('--input_type', default='AUTO', choices=opt[1],
                           help='Input format; AUTO looks at the file extension.')
        elif isinstance(opt, tuple) and opt[0] == 'db':
            p.add_argument('--db', default=opt[1], help=opt[2])
        else:
            p.add_argument('--' + opt, **_OPTIONS[opt])
    return p


def with_slash(path):
    return path if path.endswith('/') else path + '/'


_EXT = {'fq': 'fastq', 'fastq': 'fastq', 'fa': 'fasta', 'fna': 'fasta', 'fasta': 'fasta'}


def reads_kind(path, input_type):
    """The kind of a reads file: 'bam' for a BAM file (decided by its content, bam.is_bam, whatever its name or --input_type),
    else input_type, or the extension's kind when that is 'AUTO'."""
    from . import bam
    if bam.is_bam(path):
        return 'bam'
    return sniff_reads_type(path) if input_type == 'AUTO' else input_type


def sniff_reads_type(path):
    """'fastq' / 'fasta' from the extension (a trailing .gz is ignored); exits like the reference when unknown."""
    parts = path.split('.')
    ext = parts[-2] if parts[-1] == 'gz' and len(parts) > 1 else parts[-1]
    kind = _EXT.get(ext)
    if kind is None:
        sys.exit('Could not auto-determine file type. Use --input_type.')
    return kind
