"""GPU: the device inflater (mg_inflate.hip) against zlib's INFLATER on the streams of tests/deflate_writer.py — DEFLATE as zlib's compressor
never writes it (see tests/test_inflate_foreign_host.py, which runs the same corpus through the host-compiled decoder and the host
inflater): both decoders, small and large chunks, many stages and one, gzip and BGZF; what zlib refuses is refused; and a `.fq.gz` made
of such streams through the streaming entry point."""
import numpy as np
import pytest

import deflate_writer as dw

pytestmark = pytest.mark.gpu

DEFAULTS = dict(chunk_bytes=32 << 10, stage_bytes=-1, ratio=10, on=1, lane_jobs=1 << 40)


@pytest.fixture(scope="module")
def entries():
    e = dw.corpus()
    return e + dw.bgzf_forms(e)


@pytest.fixture(params=["job per wavefront", "job per lane"])
def cfg(hip, request):
    """Both decoders on every case (tests/test_gpu_inflate.py): a job per lane for launches of any size, or never."""
    try:
        hip.inflate_config(lane_jobs=0 if request.param == "job per lane" else 1 << 40)
        yield hip
    finally:
        hip.inflate_config(**DEFAULTS)


def _same(hip, blob, want, what):
    got = hip.inflate(blob)
    assert len(got) == len(want), "%s: %d bytes against %d" % (what, len(got), len(want))
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        bad = np.flatnonzero(a != b)
        raise AssertionError("%s: %d bytes differ, first at %d (got %r, want %r)" % (what, bad.size, bad[0], got[max(0, bad[0] - 20): bad[0] + 20], want[max(0, bad[0] - 20): bad[0] + 20]))


@pytest.mark.parametrize("stage", [300_000, -1])
@pytest.mark.parametrize("chunk", [8 << 10, 32 << 10])
def test_every_stream_of_the_corpus_as_zlib_reads_it(cfg, entries, chunk, stage):
    """Legal: byte-equal to zlib's text (= expand's: the corpus holds only streams on which the two agree).  Illegal: OSError.  In the
    corpus's order, so that good streams follow refused ones all the way; and one more good one at the end."""
    cfg.inflate_config(chunk_bytes=chunk, stage_bytes=stage)
    legal = refused = nbgzf = 0
    for e in entries:
        if e.want is None:
            with pytest.raises(OSError):
                cfg.inflate(e.blob)
            refused += 1
        else:
            _same(cfg, e.blob, e.want, e.name)
            legal += 1
        nbgzf += e.bgzf
    assert refused == sum(e.want is None for e in entries) and (len(entries), legal, refused, nbgzf) == (419, 353, 66, 188), (legal, refused, nbgzf)
    good = next(e for e in entries if e.name.startswith("jobs entered at a block"))
    _same(cfg, good.blob, good.want, "after the refusals")


def test_the_streams_that_span_many_chunks_are_entered_or_run_through(cfg, entries):
    """What follows from the streams themselves, whatever the finder makes of them: several stages of 300 000 bytes each; jobs entered in the
    stream whose headers only the finder's second pass accepts; the counters are printed (pytest -s) for DESIGN.md."""
    cfg.inflate_config(chunk_bytes=8 << 10, stage_bytes=300_000)
    seen = 0
    for key in ("legal headers no encoder writes", "one dynamic block of a million symbols", "megabytes of fixed and stored blocks only", "a whole .gz carried in stored blocks"):
        e = next(x for x in entries if x.name.startswith(key))
        cfg.inflate_stats(reset=True)
        _same(cfg, e.blob, e.want, e.name)
        st = cfg.inflate_stats()
        print("%s: %d compressed bytes, jobs %d, stages %d, redone %d" % (e.name, len(e.blob), st["jobs"], st["stages"], st["redone"]))
        assert st["stages"] >= 1 and st["jobs"] >= st["stages"], st
        if key.startswith("legal headers"):
            assert st["stages"] >= len(e.blob) // 300_000 and st["jobs"] > 10 * st["stages"], st  # entered in the middle: by the second pass alone
        seen += 1
    assert seen == 4


def _text_tokens(text, dists, max_len=258):
    """The text as literals and matches at the given distances only, wherever at least three bytes repeat at one (the longest)."""
    t = np.frombuffer(text, np.uint8)
    n = len(t)
    idx = np.arange(n + 1)
    best_len, best_d = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for d in dists:
        eq = np.zeros(n + 1, bool)
        eq[d:n] = t[d:] == t[:-d]
        stop = np.minimum.accumulate(np.where(~eq, idx, n)[::-1])[::-1]  # the first position from here on that does not repeat
        run = np.minimum(stop - idx, max_len)[:n]
        better = run > best_len
        best_len[better], best_d[better] = run[better], d
    cand = np.flatnonzero(best_len >= 3)
    toks, p = [], 0
    while p < n:
        j = int(np.searchsorted(cand, p))
        if j == len(cand):
            toks.append(text[p:])
            break
        q = int(cand[j])
        if q > p:
            toks.append(text[p:q])
        toks.append((int(best_len[q]), int(best_d[q])))
        p = q + int(best_len[q])
    assert dw.expand(toks) == text
    return toks


def _member(text, dists, per_block, nonstrict=False):
    """text -> a gzip member of dynamic blocks of per_block tokens: a flat code over the bytes of the text, the end of block and the length
    symbols; distance codes for the symbols of `dists` alone (one distance: one code of one bit)."""
    toks = _text_tokens(text, dists, 257 if nonstrict else 258)
    used = [sum(isinstance(t, tuple) and t[1] == d for t in toks) for d in dists]
    assert min(used) > 0, (dists, used)  # (every distance asked for is one the member's matches use)
    lsyms = sorted(set(text)) + list(range(256, 285 if nonstrict else 286))
    lit = dw.spread(286, lsyms, dw.flat_code(len(lsyms)))
    dsyms = sorted({dw.distance_symbol(d)[0] for d in dists})
    dist = dw.spread(30, dsyms, [1] * len(dsyms))
    kw = dict(hlit=286, hdist=30, hclen=19) if nonstrict else {}
    s = dw.Stream()
    for a in range(0, len(toks), per_block):
        s.dynamic(toks[a:a + per_block], lit, dist, final=a + per_block >= len(toks), **kw)
    assert s.data() == text
    return dw.gzip_member(s.raw(), text)


def test_a_streamed_fq_gz_of_foreign_streams_gives_what_the_plain_file_gives(cfg, tmp_path):
    """mg_sketch_stream_add_file on a `.fq.gz` of four members the assembler wrote — blocks with one distance code of one bit, blocks with
    distances of 32768, one block of the whole quarter, headers only the finder's second pass accepts — against the same FASTQ as a plain
    file: the same reads, the same counters.  A quarter is some 11 000 tokens and 320 KB compressed (the quality lines are one match each):
    at 250 tokens a block is about 7 KB, so that nearly every 8 KB chunk of three members holds a block start, and the third member's one
    block runs through some forty chunks that hold none.  Of inflate_stats only what follows from that is asserted (a stage of 100 000
    bytes ends at the first block boundary behind them: at most 8 stages' worth in each small-block member, 3 members of 320 KB, so more
    than 5 stages; a job at least per stage); the counters are printed (pytest -s)."""
    import test_gpu_stream as tgs
    hip = cfg
    ks = [21, 51]
    gb, go, rb, ro = tgs._sample(2, nreads=10000)
    tabs, hmaxs, filts = tgs._tables(hip, gb, go, ks)
    fq = tgs._fastq(rb, ro)
    q = len(fq) // 4
    members = [_member(fq[:q], (1,), 250), _member(fq[q:2 * q], (1, 32768), 250), _member(fq[2 * q:3 * q], (1, 32768), 1 << 30),
               _member(fq[3 * q:], (1, 20000), 250, nonstrict=True)]
    gz = b"".join(members)
    assert dw.zlib_inflate(gz) == fq and min(map(len, members)) > 300_000
    plain, packed = tmp_path / "reads.fq", tmp_path / "reads.fq.gz"
    plain.write_bytes(fq)
    packed.write_bytes(gz)
    want, wcounts = tgs._streamed(hip, ks, hmaxs, filts, rb.size, lambda st: st.add_file(str(plain), "fastq"))
    assert wcounts == (len(ro) - 1, rb.size)
    for stage in (100_000, -1):
        hip.inflate_config(chunk_bytes=8 << 10, stage_bytes=stage, on=1)
        hip.inflate_stats(reset=True)
        got, counts = tgs._streamed(hip, ks, hmaxs, filts, rb.size, lambda st: st.add_file(str(packed), "fastq"))
        assert counts == wcounts, stage
        tgs._same(got, want)
        st = hip.inflate_stats()
        print("stage_bytes %d: %d compressed bytes, jobs %d, stages %d, redone %d" % (stage, len(gz), st["jobs"], st["stages"], st["redone"]))
        assert st["jobs"] >= st["stages"] >= 1 and (stage != 100_000 or st["stages"] > 5), (stage, st)
