// mg_stream.hip — files -> HBM -> the stages, pipelined inside the library.
//
// The reference hands its reads file to `kmc` and its SAM text to a Python loop (scripts/select_db.py:43-52, `.gz` is
// expected input :146-148; scripts/map_and_profile.py:201-217).  Here the text goes through in PIECES:
//
//   reader threads      page cache -> page-locked slots (plain file: positional reads, any number of threads in
//                       parallel; gzip: zlib inflate straight into the slots — one thread for a plain gzip stream,
//                       which cannot be entered in the middle, all threads for BGZF, whose blocks say how long they are)
//   DMA stream          slot i -> device text buffer (i mod 3), behind a HEADROOM in front of which the unfinished
//                       last record (line) of piece i - 1 is placed ON THE DEVICE — so the upload of piece i + 1 does not
//                       depend on where piece i was cut and runs while piece i is parsed
//   library stream      [carry | piece] -> mg_reads_parse_prefix_dev / the SAM tokeniser -> the consumer
//                       (mg_sketch_stream_add_dev: ONE set of counting tables for the whole file)
//
// Nothing of the text ever exists as a host array beyond the slots; the host never looks at a byte of it.
//
// That is the HOST pipeline (run_pipeline).  A gzip or BGZF file has a second one, the DEVICE inflater
// (mg_inflate.hip: inflate_file_pipeline), which takes the compressed bytes up and hands the same [carry | piece] text to the
// same consumer.  stream_file chooses, once for all four entry points (reads text, BAM reads, SAM / PAF text, BAM alignments):
//
//   the file                                                             goes through
//   gzip / BGZF, whole, mg_inflate_config on, at most half of the        the device inflater; if that runs out of device
//     free device memory (and the knob inflate_dev_max_bytes)              memory before its first piece: the host pipeline
//   gzip / BGZF otherwise                                                the host pipeline: BgzfSource on all readers, or
//                                                                          ParallelGzipSource / GzipSource feeding one reader
//   plain, whole, of a kind that thins, knob stream_thin                 the host pipeline, ThinSource (*thinned = true)
//   plain otherwise (a byte range; an uncompressed BAM)                  the host pipeline, PlainSource
//
// and reader_threads says how many readers the host pipeline gets.  What an entry point adds is its StreamPlan (data), its
// consumer, a BAM file's header (skip_bam_header) and the assembly of its result.
//
// The organism files of `build_db --ingest device` are MANY files, each one genome: mg_genomes_stream (at the end of this file)
// gives every reader thread whole files and the same page-locked slots and copy stream.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#include <immintrin.h>
#endif

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "mg_inflate.h"
#include "mg_internal.h"
#include "mg_pgzip.h"

namespace mg {

// ---------------------------------------------------------------------------------------------------------------------
// byte sources
// ---------------------------------------------------------------------------------------------------------------------
struct Source {
  std::string error;  // set by fill() on failure (a reader thread must not touch the library's error text)
  int error_code = MG_ERR_ARG;
  virtual ~Source() {}
  // Piece i of the byte stream into dst (at most cap bytes).  *last = this is the stream's final piece (possibly empty).
  // Returns the bytes written, -1 on error.  Called for i = 0, 1, 2, ... — by ANY thread in any order when parallel(),
  // else by one thread in order.
  virtual int64_t fill(uint64_t i, uint8_t* dst, uint64_t cap, bool* last) = 0;
  virtual bool parallel() const = 0;
};

struct PlainSource : Source {
  int fd = -1;
  uint64_t off = 0, len = 0, cap_ = 0;
  ~PlainSource() override { if (fd >= 0) close(fd); }
  bool parallel() const override { return true; }
  int64_t fill(uint64_t i, uint8_t* dst, uint64_t cap, bool* last) override {
    const uint64_t at = i * cap;
    const uint64_t want = at >= len ? 0 : (len - at < cap ? len - at : cap);
    *last = at + want >= len;
    uint64_t got = 0;
    while (got < want) {
      const ssize_t n = pread(fd, dst + got, want - got, (off_t)(off + at + got));
      if (n < 0) { error = std::string("read failed: ") + strerror(errno); return -1; }
      if (n == 0) { error = "file is shorter than its size said"; return -1; }
      got += (uint64_t)n;
    }
    return (int64_t)got;
  }
};

// A gzip (or zlib) stream, members concatenated or not: inflated in order by ONE thread, straight into the slots.
struct GzipSource : Source {
  int fd = -1;
  z_stream zs;
  bool zs_live = false, ended = false, in_member = false, at_boundary = false;
  std::vector<uint8_t> in;
  uint64_t in_off = 0;  // file offset of the next compressed byte to read
  GzipSource() { memset(&zs, 0, sizeof(zs)); in.resize(4u << 20); }
  ~GzipSource() override { if (zs_live) inflateEnd(&zs); if (fd >= 0) close(fd); }
  bool parallel() const override { return false; }
  int64_t fill(uint64_t, uint8_t* dst, uint64_t cap, bool* last) override {
    *last = false;
    if (ended) { *last = true; return 0; }
    if (!zs_live) {
      if (inflateInit2(&zs, 15 + 32) != Z_OK) { error = "inflateInit2 failed"; return -1; }  // gzip or zlib header, detected
      zs_live = true;
    }
    zs.next_out = dst;
    uint64_t room = cap;
    while (room > 0) {
      if (zs.avail_in == 0) {
        const ssize_t n = pread(fd, in.data(), in.size(), (off_t)in_off);
        if (n < 0) { error = std::string("read failed: ") + strerror(errno); return -1; }
        if (n == 0) {  // end of the file
          if (in_member) { error = "the gzip stream ends in the middle of a member (truncated file)"; return -1; }
          ended = true;
          break;
        }
        in_off += (uint64_t)n;
        zs.next_in = in.data();
        zs.avail_in = (uInt)n;
      }
      if (at_boundary) {
        // between members only another gzip member may follow; anything else — zero padding, a tape block's fill — is
        // trailing garbage, which gzip / zcat ignore with a warning (the reference feeds `.gz` files to kmc and zcat,
        // scripts/select_db.py:105,146-148)
        if (zs.next_in[0] != 0x1f || (zs.avail_in > 1 && zs.next_in[1] != 0x8b)) { ended = true; break; }
        at_boundary = false;
      }
      zs.avail_out = (uInt)(room > 0x40000000ull ? 0x40000000ull : room);
      const uInt before = zs.avail_out;
      in_member = true;
      const int rc = inflate(&zs, Z_NO_FLUSH);
      room -= before - zs.avail_out;
      if (rc == Z_STREAM_END) {
        in_member = false;  // a member ended: another may follow (bgzip, cat a.gz b.gz, pigz -i)
        at_boundary = true;
        if (inflateReset(&zs) != Z_OK) { error = "inflateReset failed"; return -1; }
      } else if (rc != Z_OK && rc != Z_BUF_ERROR) {
        error = std::string("inflate failed: ") + (zs.msg ? zs.msg : "corrupt gzip data");
        return -1;
      }
    }
    if (ended) *last = true;
    return (int64_t)(cap - room);
  }
};

// The same stream inflated by MANY host threads (mg_pgzip.hip: deflate entered in the middle, the pugz / rapidgzip scheme):
// the decoder runs ahead in the background, one reader thread copies its output into the slots in order.
struct ParallelGzipSource : Source {
  std::unique_ptr<PGzip> g;
  bool ended = false;
  bool parallel() const override { return false; }
  int64_t fill(uint64_t, uint8_t* dst, uint64_t cap, bool* last) override {
    *last = false;
    if (ended) { *last = true; return 0; }
    const int64_t n = g->read(dst, cap);
    if (n < 0) { error = g->error(); return -1; }
    if ((uint64_t)n < cap) { ended = true; *last = true; }
    return n;
  }
};

// BGZF (bgzip / htslib): gzip members of at most 64 KB that carry their own compressed size (extra field 'BC'), so the
// file can be indexed without inflating anything and every block inflated independently — by all reader threads.
struct BgzfSource : Source {
  struct Block { uint64_t coff; uint32_t csize, isize; };
  struct Group { uint64_t first, count, bytes; };
  int fd = -1;
  std::vector<Block> blocks;
  std::vector<Group> groups;  // consecutive blocks of at most one piece together
  ~BgzfSource() override { if (fd >= 0) close(fd); }
  bool parallel() const override { return true; }

  // true when the file is BGZF from its first to its last byte (every member has the BC field); builds the index
  static bool is_bgzf_header(const uint8_t* h) {
    return h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4) && h[10] == 6 && h[11] == 0 && h[12] == 'B' && h[13] == 'C' &&
           h[14] == 2 && h[15] == 0;
  }
  bool index(uint64_t fsize, uint64_t cap) {
    uint64_t at = 0;
    uint8_t h[18], tail[4];
    while (at < fsize) {
      if (fsize - at < 28 || pread(fd, h, 18, (off_t)at) != 18 || !is_bgzf_header(h)) return false;
      const uint32_t csize = (uint32_t)(h[16] | (h[17] << 8)) + 1u;
      if (csize < 26 || at + csize > fsize) return false;
      if (pread(fd, tail, 4, (off_t)(at + csize - 4)) != 4) return false;
      const uint32_t isize = (uint32_t)tail[0] | ((uint32_t)tail[1] << 8) | ((uint32_t)tail[2] << 16) | ((uint32_t)tail[3] << 24);
      if (isize > 65536u) return false;
      blocks.push_back(Block{at, csize, isize});
      at += csize;
    }
    Group g{0, 0, 0};
    for (uint64_t b = 0; b < blocks.size(); ++b) {
      if (g.count && g.bytes + blocks[b].isize > cap) { groups.push_back(g); g = Group{b, 0, 0}; }
      ++g.count;
      g.bytes += blocks[b].isize;
    }
    groups.push_back(g);  // (an empty file has one empty group: the final piece)
    return true;
  }
  int64_t fill(uint64_t i, uint8_t* dst, uint64_t cap, bool* last) override {
    *last = i + 1 >= groups.size();
    if (i >= groups.size()) return 0;
    const Group& g = groups[i];
    if (g.bytes > cap) { error = "BGZF group larger than a slot"; return -1; }
    std::vector<uint8_t> cbuf(65536 + 64);
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) { error = "inflateInit2 failed"; return -1; }  // raw deflate: the header is skipped by hand
    uint64_t out = 0;
    for (uint64_t b = g.first; b < g.first + g.count; ++b) {
      const Block& blk = blocks[b];
      if (pread(fd, cbuf.data(), blk.csize, (off_t)blk.coff) != (ssize_t)blk.csize) { error = "short read of a BGZF block"; inflateEnd(&zs); return -1; }
      const uint32_t xlen = (uint32_t)(cbuf[10] | (cbuf[11] << 8));
      const uint32_t hdr = 12 + xlen;
      if (hdr + 8 > blk.csize) { error = "corrupt BGZF block header"; inflateEnd(&zs); return -1; }
      zs.next_in = cbuf.data() + hdr;
      zs.avail_in = blk.csize - hdr - 8;
      zs.next_out = dst + out;
      zs.avail_out = blk.isize;
      const int rc = inflate(&zs, Z_FINISH);
      if (rc != Z_STREAM_END || zs.avail_out != 0) {
        error = std::string("inflate of a BGZF block failed: ") + (zs.msg ? zs.msg : "size mismatch");
        inflateEnd(&zs);
        return -1;
      }
      out += blk.isize;
      inflateReset(&zs);
    }
    inflateEnd(&zs);
    return (int64_t)out;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// A plain FASTQ or SAM file THINNED by the reader threads to what the device parsers read.  From the page cache both
// files go up at the PCIe link's rate (3.0 + 3.5 GB per 10M reads: 0.14 s of a 0.28 s pair of command lines), and half
// of a FASTQ record (the quality line, the '+', most of the header) and two thirds of a SAM line (SEQ and QUAL, of which
// only len(SEQ) is used, scripts/map_and_profile.py:213) are never looked at on the device.
//   FASTQ  a record -> ">\n<sequence line>\n": the device parses single-line FASTA.  The reader that owns a record's
//          header line checks what k_read_lengths checks (header '@...', separator '+...') and what the parser checks
//          at the end of the file (only blank lines after the last whole record).  Which line of its record a line is
//          follows from the number of newlines in front of it: every reader counts its raw piece first and waits for
//          the counts of the pieces before it.
//   SAM    a line with at least 11 fields of str.split(): SEQ -> MG_THIN_MARK + len(SEQ) in decimal (a '*' stays),
//          QUAL -> '*'; every other byte, white space included, is kept, so the tokeniser sees the same fields, the
//          same errors and the same line numbers.  k_sam_parse takes the length from the mark (its `thin` flag).
// A raw piece is read into the slot it will leave from, behind a little room, and thinned in place (the output never
// overtakes the input: a FASTQ record shrinks, a SAM line grows by one byte only when SEQ and QUAL are one character
// each); a reader owns the lines / records that START in its piece and reads on past its end to finish the last one.
// OPT-IN (mg_debug_set("stream_thin", 1)), because it does not pay on the hosts it was measured on (profiles/r04/stream_ceilings.txt): the plain
// streams run at ~50 GB/s of text, which is the PCIe link's rate AND about what these hosts read out of the page cache at all
// (tools/pread_probe.py: 60 GB/s at four threads, less with more).  Thinning takes bytes off the link, not out of the page cache,
// and adds work per byte: with the scanner below (newline / white-space positions 32 bytes per step; the first form, one memchr per
// line, thinned 1.8 GB/s per reader) 16 readers draw level with 4 plain ones on FASTQ (0.066 s for 3.2 GB) and stay behind on SAM
// (0.097 against 0.078 s for 3.7 GB).  On a host whose memory outruns its link it is one environment variable away.
// ---------------------------------------------------------------------------------------------------------------------
static inline bool h_is_ws(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31); }

// first whitespace byte in [p, end), or end (the device's scan_to_ws: eight bytes per step)
static inline const uint8_t* h_scan_to_ws(const uint8_t* p, const uint8_t* end) {
  while (p + 8 <= end) {
    uint64_t x;
    memcpy(&x, p, 8);
    uint64_t m = (x - 0x2121212121212121ull) & ~x & 0x8080808080808080ull;
    while (m) {
      const unsigned b = (unsigned)__builtin_ctzll(m) >> 3;
      if (h_is_ws((uint8_t)(x >> (8 * b)))) return p + b;
      m &= m - 1;
    }
    p += 8;
  }
  while (p < end && !h_is_ws(*p)) ++p;
  return p;
}

// ---- candidate positions, 32 bytes per step where the host has AVX2 ----
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#define MG_HOST_AVX2 1
__attribute__((target("avx2"))) static inline uint32_t mask32_eq(const uint8_t* p, uint8_t v) {
  const __m256i x = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(p));
  return (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(x, _mm256_set1_epi8((char)v)));
}
__attribute__((target("avx2"))) static inline uint32_t mask32_le(const uint8_t* p, uint8_t v) {
  const __m256i x = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(p));
  return (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_min_epu8(x, _mm256_set1_epi8((char)v)), x));
}
static bool host_has_avx2() {  // (knob no_avx2: the byte-by-byte scanner, for the tests)
  static const bool yes = __builtin_cpu_supports("avx2") && !dbg("no_avx2");  // (read once per process)
  return yes;
}
#endif

static inline uint64_t h_count_nl(const uint8_t* p, uint64_t n) {
  uint64_t c = 0, i = 0;
#ifdef MG_HOST_AVX2
  if (host_has_avx2())
    for (; i + 32 <= n; i += 32) c += (uint64_t)__builtin_popcount(mask32_eq(p + i, '\n'));
#endif
  for (; i < n; ++i) c += p[i] == '\n';
  return c;
}

// The positions in [*, *n) of the bytes that are '\n' (LE = false) or <= 0x20 (LE = true: every white-space byte of str.split()
// is one, and a few control characters that are not), in ascending order.  *n may grow between calls (the reader reads on).
template <bool LE>
struct CandIter {
  const uint8_t* base;
  const uint64_t* n;
  uint64_t pos;    // everything below pos has been looked at
  uint64_t wbase = 0;
  uint32_t mask = 0;
  CandIter(const uint8_t* b, const uint64_t* nn, uint64_t from) : base(b), n(nn), pos(from) {}
  // the next candidate at or after the last one returned + 1; *n when there is none (so far)
  uint64_t next() {
    for (;;) {
      if (mask) {
        const unsigned bit = (unsigned)__builtin_ctz(mask);
        mask &= mask - 1;
        return wbase + bit;
      }
#ifdef MG_HOST_AVX2
      if (pos + 32 <= *n && host_has_avx2()) {
        mask = LE ? mask32_le(base + pos, 0x20) : mask32_eq(base + pos, '\n');
        wbase = pos;
        pos += 32;
        continue;
      }
#endif
      while (pos < *n) {
        const uint8_t c = base[pos++];
        if (LE ? c <= 0x20 : c == '\n') return pos - 1;
      }
      return *n;
    }
  }
  // forget what lies below `from` (the caller jumped ahead, e.g. past a record it has taken)
  void skip_to(uint64_t from) {
    if (from <= pos) {
      if (mask && from > wbase) mask &= from - wbase >= 32 ? 0u : ~((1u << (from - wbase)) - 1u);
    } else {
      mask = 0;
      pos = from;
    }
  }
};

struct ThinSource : Source {
  enum Kind { kFastq = 0, kSam = 1 };
  int fd = -1;
  Kind kind = kFastq;
  uint64_t len = 0, raw = 0, npieces = 1;
  static constexpr uint64_t kRoom = 4096;  // in front of the raw bytes: what a piece of absurd SAM lines may grow by
  // FASTQ: newlines per raw piece, as the readers come to know them
  std::mutex m;
  std::condition_variable cv;
  std::vector<int64_t> nl;
  bool dead = false;  // a reader failed: nobody waits for its count
  ~ThinSource() override { if (fd >= 0) close(fd); }
  bool parallel() const override { return true; }

  // the raw piece size for slots of `cap` bytes
  static uint64_t raw_for(uint64_t cap) {
    const uint64_t tail = cap / 4 > (4u << 20) ? (4u << 20) : cap / 4;
    return cap > kRoom + tail + 1 ? cap - kRoom - tail : 1;
  }
  void setup(uint64_t file_len, uint64_t cap) {
    len = file_len;
    raw = raw_for(cap);
    npieces = len ? (len + raw - 1) / raw : 1;
    if (kind == kFastq) nl.assign(npieces, -1);
  }
  bool read_at(uint8_t* dst, uint64_t n, uint64_t at, std::string* why) {
    uint64_t got = 0;
    while (got < n) {
      const ssize_t r = pread(fd, dst + got, n - got, (off_t)(at + got));
      if (r < 0 && errno == EINTR) continue;
      if (r < 0) { *why = std::string("read failed: ") + strerror(errno); return false; }
      if (r == 0) { *why = "file is shorter than its size said"; return false; }
      got += (uint64_t)r;
    }
    return true;
  }
  int64_t give_up(const std::string& why, int code = MG_ERR_ARG) {
    {
      std::lock_guard<std::mutex> lk(m);
      if (!dead) { error = why; error_code = code; }  // (the first failure is the one reported)
      dead = true;
    }
    cv.notify_all();
    return -1;
  }

  int64_t fill(uint64_t i, uint8_t* dst, uint64_t cap, bool* last) override {
    *last = i + 1 >= npieces;
    if (i >= npieces || len == 0) return 0;
    const uint64_t a = i * raw, b = a + raw < len ? a + raw : len;
    uint8_t* const in0 = dst + kRoom;          // raw byte a lands here; byte a - 1 right in front of it
    uint64_t have = b - a;                     // raw bytes in the slot so far: [a, a + have)
    std::string io_error;  // (this call's own: `error` belongs to whichever reader failed first)
    if (a > 0) { if (!read_at(in0 - 1, have + 1, a - 1, &io_error)) return give_up(io_error); }
    else if (!read_at(in0, have, 0, &io_error)) return give_up(io_error);
    if (kind == kFastq) {
      const int64_t c = (int64_t)h_count_nl(in0, have);
      { std::lock_guard<std::mutex> lk(m); nl[i] = c; }
      cv.notify_all();
    }
    // more of the file behind the piece, for the line / record that starts in it and ends after it
    auto more = [&]() -> int {  // 1: got some, 0: end of the file, -1: no room / error
      if (a + have >= len) return 0;
      const uint64_t room = cap - kRoom - have;
      if (room == 0) return -1;
      uint64_t n = len - (a + have);
      if (n > room) n = room;
      if (n > (256u << 10)) n = 256u << 10;
      if (!read_at(in0 + have, n, a + have, &io_error)) return -1;
      have += n;
      return 1;
    };
    const auto too_long = [&]() {
      if (!io_error.empty()) return give_up(io_error);
      return give_up("a record of more than " + std::to_string((unsigned long long)(cap - kRoom - raw)) +
                         " bytes past its piece does not fit the streaming pieces", MG_ERR_CAPACITY);
    };
    // the first line that starts in [a, b)
    uint64_t s = 0;
    const bool fresh = a == 0 || in0[-1] == '\n';
    if (!fresh) {
      const uint8_t* q = static_cast<const uint8_t*>(memchr(in0, '\n', (size_t)(b - a)));
      if (!q) return 0;  // one line runs through the whole piece: its owner is an earlier piece
      s = (uint64_t)(q - in0) + 1;
    }
    uint8_t* out = dst;
    if (kind == kSam) {
      CandIter<true> it(in0, &have, s);
      while (s < b - a) {
        // the line's fields = the gaps between its white-space bytes (str.split()); the line ends at its '\n' or with the file
        const uint8_t* lb = in0 + s;
        uint64_t prev = s;  // one past the last white-space byte seen (s: none yet)
        int nf = 0;
        uint64_t f9b = 0, f9e = 0, f10b = 0, f10e = 0, e = 0;
        bool eof = false;
        for (;;) {
          uint64_t c = it.next();
          if (c >= have) {
            const int r = more();
            if (r < 0) return too_long();
            if (r > 0) continue;
            eof = true;
            c = have;
          }
          if (!eof && !h_is_ws(in0[c])) continue;  // (a control character inside a field)
          if (c > prev) {
            if (nf == 9) { f9b = prev; f9e = c; }
            if (nf == 10) { f10b = prev; f10e = c; }
            ++nf;
          }
          prev = c + 1;
          if (eof || in0[c] == '\n') { e = c; break; }
        }
        const uint8_t* le = in0 + e;
        if (le > lb && *lb != '@' && nf >= 11) {
          const uint8_t *p9b = in0 + f9b, *p9e = in0 + f9e, *p10b = in0 + f10b, *p10e = in0 + f10e;
          const bool star = f9e - f9b == 1 && *p9b == '*';
          char num[24];
          const int nd = star ? 0 : snprintf(num, sizeof(num), "%llu", (unsigned long long)(f9e - f9b));
          // every part is written at or below where it came from as long as the rewritten SEQ ends no later than the original did
          // (it is longer only for a one-character SEQ: kRoom such lines per piece before this gives up)
          if (out + (p9b - lb) + (star ? 1 : 1 + nd) > p9e) return give_up("a piece of SAM text grew while it was thinned");
          memmove(out, lb, (size_t)(p9b - lb)); out += p9b - lb;
          if (star) *out++ = '*';
          else { *out++ = (uint8_t)MG_THIN_MARK; memcpy(out, num, (size_t)nd); out += nd; }
          memmove(out, p9e, (size_t)(p10b - p9e)); out += p10b - p9e;
          *out++ = '*';
          memmove(out, p10e, (size_t)(le - p10e)); out += le - p10e;
        } else {
          memmove(out, lb, (size_t)(le - lb)); out += le - lb;
        }
        if (!eof) *out++ = '\n';
        s = e + 1;
        if (eof) break;
      }
      return (int64_t)(out - dst);
    }
    // FASTQ: the index of the line at s = the newlines in front of it
    uint64_t before = 0;
    {
      std::unique_lock<std::mutex> lk(m);
      for (uint64_t j = 0; j < i; ++j) {
        cv.wait(lk, [&] { return dead || nl[j] >= 0; });
        if (dead) return -1;
        before += (uint64_t)nl[j];
      }
    }
    CandIter<false> it(in0, &have, s);
    // end of the line the scanner stands in: offset of its '\n', or of the end of the file (*eof); -1: no room / error
    auto line_end = [&](bool* eof) -> int64_t {
      *eof = false;
      for (;;) {
        const uint64_t c = it.next();
        if (c < have) return (int64_t)c;
        const int r = more();
        if (r < 0) return -1;
        if (r == 0) { *eof = true; return (int64_t)have; }
      }
    };
    uint64_t L = before + (fresh ? 0 : 1);
    while (s < b - a) {
      bool eof = false;
      if (L % 4 != 0) {  // a line of a record that an earlier piece owns
        const int64_t e = line_end(&eof);
        if (e < 0) return too_long();
        if (eof) break;
        s = (uint64_t)e + 1;
        ++L;
        continue;
      }
      uint64_t lb[4], le[4];
      int k = 0;
      uint64_t at = s;
      for (; k < 4; ++k) {
        const int64_t e = line_end(&eof);
        if (e < 0) return too_long();
        lb[k] = at; le[k] = (uint64_t)e;
        at = (uint64_t)e + 1;
        if (eof) { if (le[k] > lb[k]) ++k; break; }  // (nothing behind the last newline is not a line)
      }
      if (k < 4) {  // the end of the file inside a record: only blank lines may be left (the parser's rule)
        for (int j = 0; j < k; ++j) {
          const uint64_t n = le[j] - lb[j];
          if (!(n == 0 || (n == 1 && in0[lb[j]] == '\r')))
            return give_up("reads text: " + std::to_string((unsigned long long)(L + (uint64_t)k)) + " lines is not a whole number of 4-line records");
        }
        break;
      }
      auto stripped = [&](int j) { return le[j] > lb[j] && in0[le[j] - 1] == '\r' ? le[j] - 1 : le[j]; };
      if (stripped(0) == lb[0] || in0[lb[0]] != '@' || stripped(2) == lb[2] || in0[lb[2]] != '+')
        return give_up("reads file: malformed record " + std::to_string((unsigned long long)(L / 4)) + " (header / separator line)");
      *out++ = '>';
      *out++ = '\n';
      memmove(out, in0 + lb[1], (size_t)(le[1] - lb[1]));
      out += le[1] - lb[1];
      *out++ = '\n';
      s = at;
      L += 4;
      if (eof) break;
    }
    return (int64_t)(out - dst);
  }
};

static bool looks_gzip(int fd) {
  uint8_t h[2];
  return pread(fd, h, 2, 0) == 2 && h[0] == 0x1f && h[1] == 0x8b;
}

// ---------------------------------------------------------------------------------------------------------------------
// resources kept between calls (page-locking a slot costs milliseconds: the slots stay)
// ---------------------------------------------------------------------------------------------------------------------
struct StreamRes {
  hipStream_t copy = nullptr;
  std::vector<uint8_t*> slots;
  uint64_t slot_bytes = 0;
  std::vector<hipEvent_t> ev_slot;   // the DMA out of slot s has run
  hipEvent_t ev_h2d[3] = {nullptr, nullptr, nullptr};     // device buffer b holds its piece
  hipEvent_t ev_parsed[3] = {nullptr, nullptr, nullptr};  // ... and nothing reads it any more
};
static StreamRes g_res;

void stream_release_all() {
  StreamRes& r = g_res;
  if (r.copy) { (void)hipStreamSynchronize(r.copy); (void)hipStreamDestroy(r.copy); }
  for (uint8_t* p : r.slots) (void)hipHostFree(p);
  for (hipEvent_t e : r.ev_slot) (void)hipEventDestroy(e);
  for (int b = 0; b < 3; ++b) {
    if (r.ev_h2d[b]) (void)hipEventDestroy(r.ev_h2d[b]);
    if (r.ev_parsed[b]) (void)hipEventDestroy(r.ev_parsed[b]);
  }
  r = StreamRes();
}

static int ensure_res(uint64_t slot_bytes, size_t nslots) {
  StreamRes& r = g_res;
  if (!r.copy) MG_HIP(hipStreamCreateWithFlags(&r.copy, hipStreamNonBlocking));
  if (r.slot_bytes != slot_bytes) {
    for (uint8_t* p : r.slots) (void)hipHostFree(p);
    r.slots.clear();
    r.slot_bytes = slot_bytes;
  }
  while (r.slots.size() < nslots) {
    uint8_t* p = nullptr;
    MG_HIP(hipHostMalloc(reinterpret_cast<void**>(&p), slot_bytes, hipHostMallocDefault));
    r.slots.push_back(p);
  }
  while (r.ev_slot.size() < nslots) {
    hipEvent_t e = nullptr;
    MG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    r.ev_slot.push_back(e);
  }
  for (int b = 0; b < 3; ++b) {
    if (!r.ev_h2d[b]) MG_HIP(hipEventCreateWithFlags(&r.ev_h2d[b], hipEventDisableTiming));
    if (!r.ev_parsed[b]) MG_HIP(hipEventCreateWithFlags(&r.ev_parsed[b], hipEventDisableTiming));
  }
  return MG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the pipeline
// ---------------------------------------------------------------------------------------------------------------------
// consumer(d_text, nbytes, final, &consumed): the library-stream side of one piece; [consumed, nbytes) is carried.
using Consumer = std::function<int(const uint8_t*, uint64_t, bool, uint64_t*)>;

struct SlotState {
  std::mutex m;
  std::condition_variable cv;
  int64_t filled = -1;        // piece number the slot holds (ready for the DMA)
  int64_t dma_queued = -1;    // piece number whose DMA out of the slot has been queued (ev_slot recorded behind it)
  int64_t bytes = 0;
  bool last = false;
};

static int run_pipeline(Source& src, uint64_t chunk_bytes, int nthreads, const Consumer& consume, uint64_t* pieces_out) {
  Context& c = ctx();
  if (chunk_bytes < (1u << 16)) chunk_bytes = 1u << 16;
  chunk_bytes = (chunk_bytes + 4095) & ~4095ull;
  const uint64_t headroom = chunk_bytes / 4 > (4u << 20) ? chunk_bytes / 4 : (chunk_bytes < (4u << 20) ? chunk_bytes : (4u << 20));
  if (nthreads < 1) nthreads = 1;
  if (!src.parallel()) nthreads = 1;
  const size_t nslots = (size_t)nthreads + 2;
  MG_TRY(ensure_res(chunk_bytes, nslots));
  StreamRes& r = g_res;
  DevBuf dtext[3];
  for (int b = 0; b < 3; ++b) MG_TRY(dtext[b].alloc(headroom + chunk_bytes + 64));
  std::vector<std::unique_ptr<SlotState>> st(nslots);
  for (auto& p : st) p.reset(new SlotState());
  std::atomic<uint64_t> next_piece{0};
  std::atomic<bool> stop{false}, failed{false};
  std::atomic<int64_t> last_piece{-1};  // known once some reader has seen the end of the stream

  auto reader = [&]() {
    (void)hipSetDevice(c.device);
    for (;;) {
      const uint64_t i = next_piece.fetch_add(1);
      const int64_t lp = last_piece.load();
      if (stop.load() || (lp >= 0 && (int64_t)i > lp)) return;
      const size_t s = i % nslots;
      SlotState& ss = *st[s];
      if (i >= nslots) {  // the slot's previous piece must have left it
        std::unique_lock<std::mutex> lk(ss.m);
        ss.cv.wait(lk, [&] { return stop.load() || ss.dma_queued == (int64_t)(i - nslots); });
        if (stop.load()) return;
        lk.unlock();
        (void)hipEventSynchronize(r.ev_slot[s]);
      }
      bool last = false;
      const int64_t n = src.fill(i, r.slots[s], chunk_bytes, &last);
      {
        std::lock_guard<std::mutex> lk(ss.m);
        if (n < 0) { failed.store(true); ss.bytes = 0; ss.last = true; }
        else { ss.bytes = n; ss.last = last; }
        ss.filled = (int64_t)i;
      }
      if (last || n < 0) {
        int64_t expect = -1;
        last_piece.compare_exchange_strong(expect, (int64_t)i);
      }
      ss.cv.notify_all();
      if (n < 0) return;
    }
  };
  std::vector<std::thread> threads;
  for (int t = 0; t < nthreads; ++t) threads.emplace_back(reader);
  auto shut = [&]() {
    stop.store(true);
    for (auto& p : st) { std::lock_guard<std::mutex> lk(p->m); p->cv.notify_all(); }
    for (auto& t : threads) if (t.joinable()) t.join();
  };

  int rc = MG_OK;
  uint64_t carry = 0, npieces = 0;
  hipStream_t main_st = c.stream;
  // piece j's DMA is queued BEFORE piece j - 1 is parsed: the copy engine works while this thread waits in the parser
  auto queue_dma = [&](uint64_t j, int64_t* bytes, bool* last) -> int {
    const size_t s = j % nslots;
    const int b = (int)(j % 3);
    SlotState& ss = *st[s];
    {
      std::unique_lock<std::mutex> lk(ss.m);
      ss.cv.wait(lk, [&] { return ss.filled == (int64_t)j; });
      *bytes = ss.bytes;
      *last = ss.last;
    }
    if (failed.load()) return fail(src.error_code, "%s", src.error.empty() ? "reading the input failed" : src.error.c_str());
    if (j >= 3) MG_HIP(hipStreamWaitEvent(r.copy, r.ev_parsed[b], 0));  // the buffer's previous piece has been parsed
    if (*bytes > 0)
      MG_HIP(hipMemcpyAsync(dtext[b].as<uint8_t>() + headroom, r.slots[s], (size_t)*bytes, hipMemcpyHostToDevice, r.copy));
    MG_HIP(hipEventRecord(r.ev_slot[s], r.copy));
    MG_HIP(hipEventRecord(r.ev_h2d[b], r.copy));
    {
      std::lock_guard<std::mutex> lk(ss.m);
      ss.dma_queued = (int64_t)j;
    }
    ss.cv.notify_all();
    return MG_OK;
  };

  int64_t cur_bytes = 0, nxt_bytes = 0;
  bool cur_last = false, nxt_last = false;
  rc = queue_dma(0, &cur_bytes, &cur_last);
  for (uint64_t j = 0; rc == MG_OK; ++j) {
    if (!cur_last) rc = queue_dma(j + 1, &nxt_bytes, &nxt_last);
    if (rc != MG_OK) break;
    const int b = (int)(j % 3);
    rc = hipStreamWaitEvent(main_st, r.ev_h2d[b], 0) == hipSuccess ? MG_OK : fail(MG_ERR_HIP, "hipStreamWaitEvent failed");
    if (rc != MG_OK) break;
    const uint8_t* text = dtext[b].as<uint8_t>() + headroom - carry;
    const uint64_t nbytes = carry + (uint64_t)cur_bytes;
    uint64_t consumed = 0;
    rc = consume(text, nbytes, cur_last, &consumed);
    if (rc != MG_OK) break;
    ++npieces;
    if (cur_last) break;
    if (consumed > nbytes) consumed = nbytes;
    const uint64_t left = nbytes - consumed;
    if (left > headroom) {
      rc = fail(MG_ERR_CAPACITY, "a record of more than %llu bytes does not fit the streaming pieces", (unsigned long long)headroom);
      break;
    }
    if (left) {
      const int nb = (int)((j + 1) % 3);
      if (hipMemcpyAsync(dtext[nb].as<uint8_t>() + headroom - left, text + consumed, (size_t)left, hipMemcpyDeviceToDevice, main_st) != hipSuccess) {
        rc = fail(MG_ERR_HIP, "carry copy failed");
        break;
      }
    }
    carry = left;
    if (hipEventRecord(r.ev_parsed[b], main_st) != hipSuccess) { rc = fail(MG_ERR_HIP, "hipEventRecord failed"); break; }
    cur_bytes = nxt_bytes;
    cur_last = nxt_last;
  }
  shut();
  (void)hipStreamSynchronize(r.copy);
  if (rc != MG_OK) (void)hipStreamSynchronize(main_st);  // (what was queued may still read the buffers released below)
  if (pieces_out) *pieces_out = npieces;
  return rc;
}

// *chunk_bytes: 0 = the default of the source's kind (32 MB: tools/stream_probe.py — 3.2 GB of FASTQ, 8 readers: 16 MB pieces
// 0.089 s, 32 MB 0.071 s, 64 MB 0.067 s warm, but 0.105 against 0.122 s with the page-locked slots still to be allocated, which is
// what a one-shot command line pays; BGZF 16 MB: many inflating threads, each with a slot).
// thin_kind: -1, or what a plain file read from its first to its last byte may be thinned as (ThinSource::Kind); *thinned tells.
static int open_source(const char* path, uint64_t offset, uint64_t length, uint64_t* chunk_bytes, std::unique_ptr<Source>* out, bool* gz,
                       int thin_kind = -1, bool* thinned = nullptr) {
  if (thinned) *thinned = false;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return fail(MG_ERR_ARG, "cannot open %s: %s", path, strerror(errno));
  struct stat sb;
  if (fstat(fd, &sb) != 0) { close(fd); return fail(MG_ERR_ARG, "cannot stat %s", path); }
  const uint64_t fsize = (uint64_t)sb.st_size;
  *gz = looks_gzip(fd);
  if (*gz) {
    if (offset || length) { close(fd); return fail(MG_ERR_ARG, "a byte range of a gzip file cannot be streamed"); }
    std::unique_ptr<BgzfSource> bz(new BgzfSource());
    bz->fd = fd;
    uint64_t bc = *chunk_bytes ? *chunk_bytes : (16ull << 20);
    if (bc < (1u << 16)) bc = 1u << 16;
    if (bz->index(fsize, bc)) { *chunk_bytes = bc; *out = std::move(bz); return MG_OK; }
    bz->fd = -1;  // not BGZF: one deflate stream
    if (!*chunk_bytes) *chunk_bytes = 32ull << 20;
    unsigned hw = std::thread::hardware_concurrency();
    int threads = (int)(hw == 0 ? 4 : (hw > 64 ? 64 : hw));
    if (dbg("gzip_threads") > 0) threads = (int)dbg("gzip_threads");
    if (threads > 1) {
      // ... entered in the middle by every core the box has (knob gzip_threads = 1: zlib, one thread, as rounds 2-3)
      std::string err;
      uint64_t pc = 1ull << 20;
      if (threads > 32) threads = 32;  // (two chunks per thread in flight, ~15 MB each inflated: a gigabyte of host memory at 32)
      if (dbg("pgzip_chunk") > 0) pc = (uint64_t)dbg("pgzip_chunk");
      std::unique_ptr<ParallelGzipSource> pg(new ParallelGzipSource());
      pg->g = PGzip::open(fd, true, fsize, threads, pc, &err);
      if (!pg->g) { close(fd); return fail(MG_ERR_ARG, "%s: %s", path, err.c_str()); }
      *out = std::move(pg);
      return MG_OK;
    }
    std::unique_ptr<GzipSource> g(new GzipSource());
    g->fd = fd;
    *out = std::move(g);
    return MG_OK;
  }
  if (offset > fsize) { close(fd); return fail(MG_ERR_ARG, "offset beyond the end of %s", path); }
  if (!*chunk_bytes) *chunk_bytes = 32ull << 20;
  if (thin_kind >= 0 && thinned && offset == 0 && length == 0) {
    if (dbg("stream_thin")) {  // opt-in: see the note at ThinSource
      uint64_t cb = *chunk_bytes < (1u << 16) ? (1u << 16) : *chunk_bytes;  // (the pipeline's own rounding of the slot size)
      cb = (cb + 4095) & ~4095ull;
      std::unique_ptr<ThinSource> t(new ThinSource());
      t->fd = fd;
      t->kind = thin_kind == 0 ? ThinSource::kFastq : ThinSource::kSam;
      t->setup(fsize, cb);
      *thinned = true;
      *out = std::move(t);
      return MG_OK;
    }
  }
  std::unique_ptr<PlainSource> p(new PlainSource());
  p->fd = fd;
  p->off = offset;
  p->len = length ? (offset + length > fsize ? fsize - offset : length) : fsize - offset;
  *out = std::move(p);
  return MG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the driver: this file's bytes, as pieces of text on the device, to this consumer (the decision table is at the top of the file)
// ---------------------------------------------------------------------------------------------------------------------
// What differs between the entry points — data, not code.
struct StreamPlan {
  uint64_t offset = 0, length = 0;  // a byte range of a plain file (0, 0: the whole file)
  uint64_t chunk_bytes = 0;         // 0: the default of the source's kind (open_source)
  int nthreads = 0;                 // <= 0: reader_threads decides
  int thin_kind = -1;               // -1, or the ThinSource::Kind a plain whole file may be thinned as
  // The host readers of a BGZF file, when the caller named no number: every core (up to 32), because inflating is the work —
  // or the eight of any other file.  The entry points differ, and every figure was taken with these values:
  //   mg_sketch_stream_add_file, text   true       bam_reads_file       true
  //   mg_sam_stream_file                false      mg_bam_stream_file   false
  bool bgzf_uses_all_cores = false;
  // ... and also when the caller DID name a number (mg_sketch_stream_add_file's text formats only: the tests and the probes under
  // tools/ that pass thread counts measure this)
  bool bgzf_overrides_caller = false;
};

// The reader threads of the host pipeline (run_pipeline itself takes one for a source that is not parallel()).
static int reader_threads(const StreamPlan& plan, bool bgzf, bool thinned) {
  const unsigned hw = std::thread::hardware_concurrency();
  const bool auto_threads = plan.nthreads <= 0;
  if (dbg("stream_threads") > 0) return auto_threads ? (int)dbg("stream_threads") : plan.nthreads;  // (the knob fixes the number)
  int n = auto_threads ? (int)(hw == 0 ? 4 : (hw > 8 ? 8 : hw)) : plan.nthreads;
  if (bgzf && plan.bgzf_uses_all_cores && (auto_threads || plan.bgzf_overrides_caller) && hw > (unsigned)n) n = (int)(hw > 32 ? 32 : hw);
  // Thinning is host work per byte (a reader does ~4 GB/s of it against ~12 GB/s of plain reads): twice the readers, when the
  // box has twice as many cores again and nobody fixed the number.
  if (thinned && auto_threads && hw >= (unsigned)n * 4) n *= 2;
  return n;
}

// A `.gz` file (gzip or BGZF) whose compressed bytes go to the device and are inflated there (mg_inflate.hip), unless
// mg_inflate_config turned that off: -> fd >= 0 and its size; -1: not such a file (the host readers take it)
// (... or too large a file: the device inflater holds the WHOLE compressed file in device memory beside the pieces of text in
// flight; a file above half of what is free — or above the knob inflate_dev_max_bytes — goes through the host inflater, whose
// memory is bounded by its pieces.)
static int open_for_device_inflate(const char* path, uint64_t offset, uint64_t length, uint64_t* fsize) {
  if (!inflate_dev_enabled() || offset || length) return -1;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return -1;
  struct stat sb;
  if (fstat(fd, &sb) != 0 || !looks_gzip(fd)) { close(fd); return -1; }
  *fsize = (uint64_t)sb.st_size;
  size_t free_b = 0, total_b = 0;
  uint64_t cap = hipMemGetInfo(&free_b, &total_b) == hipSuccess ? (uint64_t)free_b / 2 : 0;
  if (dbg("inflate_dev_max_bytes") > 0 && (uint64_t)dbg("inflate_dev_max_bytes") < cap) cap = (uint64_t)dbg("inflate_dev_max_bytes");
  if (*fsize > cap) { close(fd); return -1; }
  return fd;
}

// *thinned (may be null) is set before the first call of `consume`: the consumer may read it through a captured reference.
// The device inflater running out of memory (MG_ERR_NOMEM) before it handed over its first piece is no error: `consume` has not
// been called, so whatever state it keeps is untouched, and the host readers take the file from its first byte.  That holds for
// the compressed file's own buffer and for everything the inflater sets up behind it, for every entry point.
static int stream_file(const char* path, const StreamPlan& plan, const Consumer& consume, bool* thinned = nullptr) {
  bool thinned_here = false;
  if (!thinned) thinned = &thinned_here;
  *thinned = false;
  uint64_t fsize = 0;
  const int gfd = open_for_device_inflate(path, plan.offset, plan.length, &fsize);
  if (gfd >= 0) {
    bool started = false;
    const int rc = inflate_file_pipeline(gfd, fsize, consume, &started);
    close(gfd);
    if (!(rc == MG_ERR_NOMEM && !started)) return rc;
  }
  std::unique_ptr<Source> src;
  bool gz = false;
  uint64_t chunk_bytes = plan.chunk_bytes;
  MG_TRY(open_source(path, plan.offset, plan.length, &chunk_bytes, &src, &gz, plan.thin_kind, thinned));
  return run_pipeline(*src, chunk_bytes, reader_threads(plan, gz && src->parallel(), *thinned), consume, nullptr);
}

// `inner` behind a BAM file's header (read by the caller with zlib: hdr_bytes of the inflated stream): its bytes are eaten from
// the first piece(s), and inner sees the records only.
static Consumer skip_bam_header(uint64_t hdr_bytes, const char* path, Consumer inner) {
  return [skip = hdr_bytes, path, inner = std::move(inner)](const uint8_t* d_text, uint64_t nbytes, bool final, uint64_t* consumed) mutable -> int {
    const uint64_t off = skip < nbytes ? skip : nbytes;  // the header's bytes
    skip -= off;
    if (skip) {
      *consumed = nbytes;
      return final ? fail(MG_ERR_ARG, "%s: the BAM header runs past the end of the file", path) : MG_OK;
    }
    uint64_t used = 0;
    MG_TRY(inner(d_text + off, nbytes - off, final, &used));
    *consumed = off + used;
    return MG_OK;
  };
}

// A BAM READS file (BGZF, or uncompressed) -> its reads, piece by piece: the header read here with zlib and stepped over, every
// piece cut after its last complete record, its records unpacked on the device (mg_bam.hip: bam_reads_prefix_dev).  sink(reads)
// owns each batch.  A break in the record chain: MG_ERR_ARG naming the file and the byte of the inflated stream.
static int bam_reads_file(const char* path, uint64_t chunk_bytes, int nthreads, const std::function<int(mg_reads*)>& sink) {
  BamHeader hdr;
  MG_TRY(bam_read_header(path, &hdr));
  const int32_t n_ref = (int32_t)hdr.names.size();
  uint64_t done = hdr.bytes;  // the stream's bytes in front of this piece's records
  // (BGZF on every core, as the reads text — but a caller's own number holds)
  const StreamPlan plan{.chunk_bytes = chunk_bytes, .nthreads = nthreads, .bgzf_uses_all_cores = true};
  const int rc = stream_file(path, plan, skip_bam_header(hdr.bytes, path, [&](const uint8_t* d_recs, uint64_t nbytes, bool final, uint64_t* consumed) -> int {
    mg_reads* rd = nullptr;
    uint64_t at = 0;
    const int prc = bam_reads_prefix_dev(d_recs, nbytes, n_ref, final, consumed, &rd, &at);
    if (prc == MG_ERR_ARG) {
      const std::string why = mg_last_error();
      return fail(MG_ERR_ARG, "%s: corrupt or truncated BAM at byte %llu of the inflated stream (%s)", path,
                  (unsigned long long)(done + at), why.c_str());
    }
    MG_TRY(prc);
    done += *consumed;
    return sink(rd);
  }));
  if (rc == MG_ERR_CAPACITY) {  // (a record longer than a piece's headroom — or a corrupt block_size that claims one)
    const std::string why = mg_last_error();
    return fail(MG_ERR_CAPACITY, "%s: %s", path, why.c_str());
  }
  return rc;
}

// A batch of reads into the counting tables of the whole file; the batch is released.
static int add_reads(mg_sketch_stream* ss, mg_reads* rd) {
  const uint8_t* d_b = nullptr;
  const uint64_t* d_o = nullptr;
  int rc = mg_reads_device_ptrs(rd, &d_b, &d_o);
  if (rc == MG_OK) rc = mg_sketch_stream_add_dev(ss, d_b, d_o, mg_reads_count(rd), mg_reads_nbases(rd));
  mg_reads_free(rd);  // (stream-ordered: the hashing kernel queued above still reads it; the pool hands it out behind that)
  return rc;
}

__global__ __launch_bounds__(256) void k_shift_offsets(const uint64_t* __restrict__ in, uint64_t n, uint64_t add, uint64_t* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = in[i] + add;
}

// a piece's entries behind the pieces before it: out[i] = in[i] with off moved up by `add` where the entry is piled
__global__ __launch_bounds__(256) void k_shift_bases(const mg_aln_bases* __restrict__ in, uint64_t n, uint64_t add, mg_aln_bases* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    mg_aln_bases e = in[i];
    if (e.span) e.off += add;
    out[i] = e;
  }
}

}  // namespace mg

using namespace mg;

extern "C" {

int mg_sketch_stream_add_file(mg_sketch_stream* ss, const char* path, int format, uint64_t offset, uint64_t length,
                              uint64_t chunk_bytes, int nthreads) {
  MG_REQUIRE_READY();
  if (!ss || !path) return fail(MG_ERR_ARG, "null argument");
  if (format < 0 || format > 3) return fail(MG_ERR_ARG, "format must be 0 (fastq), 1 (single-line fasta), 2 (fasta) or 3 (bam)");
  if (format == 3) {
    if (offset || length) return fail(MG_ERR_ARG, "a byte range of a BAM file cannot be streamed");
    return bam_reads_file(path, chunk_bytes, nthreads, [&](mg_reads* rd) -> int { return add_reads(ss, rd); });
  }
  // (BGZF: inflating is the work — every core the box has, whatever the caller asked for)
  const StreamPlan plan{.offset = offset, .length = length, .chunk_bytes = chunk_bytes, .nthreads = nthreads,
                        .thin_kind = format == 0 ? (int)ThinSource::kFastq : -1, .bgzf_uses_all_cores = true, .bgzf_overrides_caller = true};
  bool thinned = false;
  return stream_file(path, plan, [&](const uint8_t* d_text, uint64_t nbytes, bool final, uint64_t* consumed) -> int {
    const int dev_format = thinned ? 1 : format;  // (a thinned FASTQ piece is single-line FASTA: ">", the sequence line)
    mg_reads* rd = nullptr;
    MG_TRY(mg_reads_parse_prefix_dev(d_text, nbytes, dev_format, final ? 1 : 0, consumed, &rd));
    return add_reads(ss, rd);
  }, &thinned);
}

// A whole BAM reads file -> one batch (the multi-rank path: rank 0 decodes, then shares the reads out)
int mg_reads_from_bam_file(const char* path, uint64_t chunk_bytes, int nthreads, mg_reads** out) {
  MG_REQUIRE_READY();
  if (!path || !out) return fail(MG_ERR_ARG, "null argument");
  *out = nullptr;
  std::vector<std::unique_ptr<mg_reads>> parts;
  uint64_t nreads = 0, nbases = 0;
  MG_TRY(bam_reads_file(path, chunk_bytes, nthreads, [&](mg_reads* rd) -> int {
    nreads += rd->nreads;
    nbases += rd->nbases;
    parts.emplace_back(rd);
    return MG_OK;
  }));
  if (parts.size() == 1) {
    *out = parts[0].release();
    return MG_OK;
  }
  std::unique_ptr<mg_reads> all(new mg_reads());
  all->nreads = nreads;
  all->nbases = nbases;
  MG_TRY(all->offsets.alloc((nreads + 2) * sizeof(uint64_t)));
  MG_TRY(all->bases.alloc(nbases + 16));
  hipStream_t st = ctx().stream;
  MG_HIP(hipMemsetAsync(all->offsets.p, 0, sizeof(uint64_t), st));  // (offsets[0]; no parts at all: an empty batch)
  uint64_t r = 0, b = 0;
  for (auto& p : parts) {
    if (p->nbases) MG_HIP(hipMemcpyAsync(all->bases.as<uint8_t>() + b, p->bases.p, p->nbases, hipMemcpyDeviceToDevice, st));
    // (offsets[1 .. n] of the part, shifted by the bases in front of it: its offsets[0] = 0 is the previous part's last)
    if (p->nreads)
      hipLaunchKernelGGL(k_shift_offsets, dim3(grid_for(p->nreads, 256, 1024)), dim3(256), 0, st, p->offsets.as<uint64_t>() + 1,
                         p->nreads, b, all->offsets.as<uint64_t>() + r + 1);
    MG_HIP(hipGetLastError());
    r += p->nreads;
    b += p->nbases;
  }
  MG_HIP(hipStreamSynchronize(st));
  *out = all.release();
  return MG_OK;
}

// The batches of a file's pieces -> one (a single piece's records are taken over as they are); keyed pieces: their keys likewise
// named pieces: their names appended, their offsets moved up by the bytes in front of them (a read that goes on into the next
// piece opens no read there, so it is named once)
static int concat_batches(std::vector<std::unique_ptr<mg_sam_batch>>& parts, uint64_t total, const std::string& prev, bool keyed,
                          mg_sam_batch** out, bool named = false, bool placed = false, bool edited = false, bool based = false) {
  std::unique_ptr<mg_sam_batch> all(new mg_sam_batch());
  all->last_qname = prev;
  all->nrecs = total;
  all->keyed = keyed;
  if (named && parts.empty()) MG_TRY(names_empty(all.get()));
  if (placed && parts.empty()) MG_TRY(places_empty(all.get()));
  if (edited && parts.empty()) MG_TRY(edits_empty(all.get()));
  if (based && parts.empty()) MG_TRY(bases_empty(all.get()));
  if (parts.size() == 1) {
    all->recs = std::move(parts[0]->recs);
    all->keys = std::move(parts[0]->keys);
    all->name_off = std::move(parts[0]->name_off);
    all->name_bytes = std::move(parts[0]->name_bytes);
    all->nreads = parts[0]->nreads;
    all->nname_bytes = parts[0]->nname_bytes;
    all->named = parts[0]->named;
    all->places = std::move(parts[0]->places);
    all->placed = parts[0]->placed;
    all->edits = std::move(parts[0]->edits);
    all->edited = parts[0]->edited;
    all->bases = std::move(parts[0]->bases);
    all->pool = std::move(parts[0]->pool);
    all->npool = parts[0]->npool;
    all->based = parts[0]->based;
  } else {
    MG_TRY(all->recs.alloc((total + 1) * sizeof(mg_aln_rec)));
    if (keyed) MG_TRY(all->keys.alloc((total + 1) * 2 * sizeof(uint64_t)));
    if (placed && !parts.empty()) {  // the pieces' places, joined in record order like the keys
      MG_TRY(all->places.alloc((total + 1) * sizeof(mg_aln_place)));
      all->placed = true;
    }
    if (edited && !parts.empty()) {  // ... and their edits
      MG_TRY(all->edits.alloc((total + 1) * sizeof(mg_aln_edit)));
      all->edited = true;
    }
    uint64_t at = 0, pool_at = 0;
    hipStream_t st = ctx().stream;
    if (based && !parts.empty()) {  // ... and their entries, each piece's pool behind the pools before it
      uint64_t npool = 0;
      for (auto& p : parts) npool += p->npool;
      MG_TRY(all->bases.alloc((total + 1) * sizeof(mg_aln_bases)));
      MG_TRY(all->pool.alloc(npool + 16));
      all->npool = npool;
      all->based = true;
    }
    for (auto& p : parts) {
      if (based && p->nrecs) {
        hipLaunchKernelGGL(k_shift_bases, dim3(grid_for(p->nrecs, 256, 1024)), dim3(256), 0, st, p->bases.as<mg_aln_bases>(), p->nrecs, pool_at,
                           all->bases.as<mg_aln_bases>() + at);
        MG_HIP(hipGetLastError());
      }
      if (based && p->npool)
        MG_HIP(hipMemcpyAsync(all->pool.as<uint8_t>() + pool_at, p->pool.p, p->npool, hipMemcpyDeviceToDevice, st));
      if (based) pool_at += p->npool;
      if (p->nrecs)
        MG_HIP(hipMemcpyAsync(all->recs.as<mg_aln_rec>() + at, p->recs.p, p->nrecs * sizeof(mg_aln_rec), hipMemcpyDeviceToDevice, st));
      if (p->nrecs && keyed)
        MG_HIP(hipMemcpyAsync(all->keys.as<uint64_t>() + 2 * at, p->keys.p, p->nrecs * 2 * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
      if (placed && p->nrecs)
        MG_HIP(hipMemcpyAsync(all->places.as<mg_aln_place>() + at, p->places.p, p->nrecs * sizeof(mg_aln_place), hipMemcpyDeviceToDevice, st));
      if (edited && p->nrecs)
        MG_HIP(hipMemcpyAsync(all->edits.as<mg_aln_edit>() + at, p->edits.p, p->nrecs * sizeof(mg_aln_edit), hipMemcpyDeviceToDevice, st));
      at += p->nrecs;
    }
    if (named && !parts.empty()) {
      uint64_t nreads = 0, nbytes = 0;
      for (auto& p : parts) { nreads += p->nreads; nbytes += p->nname_bytes; }
      MG_TRY(all->name_off.alloc((nreads + 2) * sizeof(uint64_t)));
      MG_TRY(all->name_bytes.alloc(nbytes + 16));
      MG_HIP(hipMemsetAsync(all->name_off.p, 0, sizeof(uint64_t), st));
      uint64_t r = 0, b = 0;
      for (auto& p : parts) {
        if (p->nname_bytes)
          MG_HIP(hipMemcpyAsync(all->name_bytes.as<uint8_t>() + b, p->name_bytes.p, p->nname_bytes, hipMemcpyDeviceToDevice, st));
        if (p->nreads)
          hipLaunchKernelGGL(k_shift_offsets, dim3(grid_for(p->nreads, 256, 1024)), dim3(256), 0, st, p->name_off.as<uint64_t>() + 1,
                             p->nreads, b, all->name_off.as<uint64_t>() + r + 1);
        MG_HIP(hipGetLastError());
        r += p->nreads;
        b += p->nname_bytes;
      }
      all->nreads = nreads;
      all->nname_bytes = nbytes;
      all->named = true;
    }
    MG_HIP(hipStreamSynchronize(st));
  }
  *out = all.release();
  return MG_OK;
}

// ... and, for the collated entry points, regrouped by read (mg_collate.hip).  The knob collate_defer (a test hook) leaves the
// batch as it was tokenised, keys and all, for the caller to look at and collate (mg_sam_batch_collate_dev).
static int finish_batches(std::vector<std::unique_ptr<mg_sam_batch>>& parts, uint64_t total, const std::string& prev, bool collate,
                          mg_sam_batch** out, bool named = false, bool placed = false, bool edited = false, bool based = false) {
  mg_sam_batch* all = nullptr;
  MG_TRY(concat_batches(parts, total, prev, collate, &all, named, placed, edited, based));
  if (collate && !dbg("collate_defer")) {
    parts.clear();  // (the pieces' buffers go back to the pool before the sort asks for its own)
    const int rc = collate_batch(all, nullptr);
    if (rc != MG_OK) { delete all; return rc; }
  }
  *out = all;
  return MG_OK;
}

// SAM (paf = 0) or PAF text file -> alignment records on the device, through the same pipeline: every piece is cut at its
// last newline, tokenised (mg_sam_tokenize_dev's rules; the previous retained QNAME carried from piece to piece so that
// the new-read bit is the whole file's) and its records appended.  Replaces the per-line Python of map_and_process,
// scripts/map_and_profile.py:201-217.  A line the reference cannot parse: MG_ERR_ARG with err_kind (the caller streams
// the file through the host tokeniser, which raises what the reference raises).
static int sam_stream_file_impl(const char* path, int paf, const mg_acc_index* ix, uint64_t offset, uint64_t length,
                                uint64_t chunk_bytes, int nthreads, mg_sam_batch** out, int* err_kind, uint64_t* err_line, bool collate,
                                bool named = false, bool placed = false, bool edited = false, bool based = false) {
  MG_REQUIRE_READY();
  if (!path || !ix || !out) return fail(MG_ERR_ARG, "null argument");
  *out = nullptr;
  if (err_kind) *err_kind = 0;
  if (err_line) *err_line = 0;
  // (a BGZF file's host readers stay at the eight of a plain file)
  const StreamPlan plan{.offset = offset, .length = length, .chunk_bytes = chunk_bytes, .nthreads = nthreads,
                        .thin_kind = (paf || based) ? -1 : (int)ThinSource::kSam,  // (thinning drops SEQ)
                        .bgzf_uses_all_cores = false};
  bool thinned = false;
  std::vector<std::unique_ptr<mg_sam_batch>> parts;
  std::string prev;
  uint64_t total = 0;
  MG_TRY(stream_file(path, plan, [&](const uint8_t* d_text, uint64_t nbytes, bool final, uint64_t* consumed) -> int {
    mg_sam_batch* b = nullptr;
    MG_TRY(aln_tokenize_prefix_dev(d_text, nbytes, ix, prev.c_str(), paf != 0, final, consumed, &b, err_kind, err_line, thinned, collate, named, placed, edited, based));
    prev = b->last_qname;
    total += b->nrecs;
    parts.emplace_back(b);
    return MG_OK;
  }, &thinned));
  return finish_batches(parts, total, prev, collate, out, named, placed, edited, based);
}

// The flag-taking streams (MG_BATCH_*): KEYS alone keeps the keys on the batch (as the knob collate_defer does for a collated call).
static int stream_want_check(unsigned want, int paf) {
  if (want & ~(MG_BATCH_KEYS | MG_BATCH_NAMES | MG_BATCH_PLACES | MG_BATCH_COLLATE | MG_BATCH_EDITS | MG_BATCH_BASES)) return fail(MG_ERR_ARG, "unknown bits in want");
  if ((want & MG_BATCH_BASES) && paf) return fail(MG_ERR_ARG, "a PAF line has no CIGAR and SEQ columns: no bases from PAF");
  if ((want & MG_BATCH_PLACES) && paf) return fail(MG_ERR_ARG, "a PAF line has no POS and CIGAR columns: no places from PAF");
  if ((want & MG_BATCH_EDITS) && paf) return fail(MG_ERR_ARG, "no edits from PAF (its NM:i: and cg:Z: tags are not read)");
  if ((want & MG_BATCH_NAMES) && (want & MG_BATCH_COLLATE))
    return fail(MG_ERR_STATE, "a named batch is not collated (its names are in the order the reads came in)");
  if ((want & MG_BATCH_KEYS) && !(want & MG_BATCH_COLLATE))
    return fail(MG_ERR_ARG, "a file stream keeps the keys only to collate by them (MG_BATCH_COLLATE)");
  return MG_OK;
}

int mg_sam_stream_file_ex(const char* path, int paf, const mg_acc_index* ix, uint64_t offset, uint64_t length,
                          uint64_t chunk_bytes, int nthreads, mg_sam_batch** out, int* err_kind, uint64_t* err_line, unsigned want) {
  MG_TRY(stream_want_check(want, paf));
  return sam_stream_file_impl(path, paf, ix, offset, length, chunk_bytes, nthreads, out, err_kind, err_line,
                              (want & MG_BATCH_COLLATE) != 0, (want & MG_BATCH_NAMES) != 0, (want & MG_BATCH_PLACES) != 0,
                              (want & MG_BATCH_EDITS) != 0, (want & MG_BATCH_BASES) != 0);
}

int mg_sam_stream_file_named(const char* path, int paf, const mg_acc_index* ix, uint64_t offset, uint64_t length,
                             uint64_t chunk_bytes, int nthreads, mg_sam_batch** out, int* err_kind, uint64_t* err_line) {
  return sam_stream_file_impl(path, paf, ix, offset, length, chunk_bytes, nthreads, out, err_kind, err_line, false, true);
}

int mg_sam_stream_file(const char* path, int paf, const mg_acc_index* ix, uint64_t offset, uint64_t length,
                       uint64_t chunk_bytes, int nthreads, mg_sam_batch** out, int* err_kind, uint64_t* err_line) {
  return sam_stream_file_impl(path, paf, ix, offset, length, chunk_bytes, nthreads, out, err_kind, err_line, false);
}

int mg_sam_stream_file_collated(const char* path, int paf, const mg_acc_index* ix, uint64_t offset, uint64_t length,
                                uint64_t chunk_bytes, int nthreads, mg_sam_batch** out, int* err_kind, uint64_t* err_line) {
  return sam_stream_file_impl(path, paf, ix, offset, length, chunk_bytes, nthreads, out, err_kind, err_line, true);
}

// BAM file (BGZF, or uncompressed) -> alignment records on the device: the SAME pipeline and the same inflaters as a `.sam.gz`,
// the header read here with zlib and stepped over in the first piece(s), every piece cut after its last complete record
// (mg_bam.hip).
static int bam_stream_file_impl(const char* path, const mg_acc_index* ix, uint64_t chunk_bytes, int nthreads, mg_sam_batch** out,
                                int* err_kind, uint64_t* err_rec, bool collate, bool named = false, bool placed = false,
                                bool edited = false, bool based = false) {
  MG_REQUIRE_READY();
  if (!path || !ix || !out) return fail(MG_ERR_ARG, "null argument");
  *out = nullptr;
  if (err_kind) *err_kind = 0;
  if (err_rec) *err_rec = 0;
  BamHeader hdr;
  MG_TRY(bam_read_header(path, &hdr));
  const std::vector<int32_t> map = bam_refmap(hdr.names, ix);
  DevBuf d_map;
  MG_TRY(d_map.alloc(map.size() * sizeof(int32_t)));
  MG_TRY(mg_memcpy_h2d(d_map.p, map.data(), map.size() * sizeof(int32_t)));
  // (BGZF host readers as mg_sam_stream_file)
  const StreamPlan plan{.chunk_bytes = chunk_bytes, .nthreads = nthreads, .bgzf_uses_all_cores = false};
  std::vector<std::unique_ptr<mg_sam_batch>> parts;
  std::string prev;
  uint64_t total = 0;
  MG_TRY(stream_file(path, plan, skip_bam_header(hdr.bytes, path, [&](const uint8_t* d_recs, uint64_t nbytes, bool final, uint64_t* consumed) -> int {
    mg_sam_batch* b = nullptr;
    MG_TRY(bam_tokenize_prefix_dev(d_recs, nbytes, d_map.as<int32_t>(), (int32_t)hdr.names.size(), prev.c_str(), final, consumed, &b,
                                   err_kind, err_rec, collate, named, placed, edited, based));
    prev = b->last_qname;
    total += b->nrecs;
    parts.emplace_back(b);
    return MG_OK;
  })));
  return finish_batches(parts, total, prev, collate, out, named, placed, edited, based);
}

int mg_bam_stream_file_ex(const char* path, const mg_acc_index* ix, uint64_t chunk_bytes, int nthreads, mg_sam_batch** out,
                          int* err_kind, uint64_t* err_rec, unsigned want) {
  MG_TRY(stream_want_check(want, 0));
  return bam_stream_file_impl(path, ix, chunk_bytes, nthreads, out, err_kind, err_rec, (want & MG_BATCH_COLLATE) != 0,
                              (want & MG_BATCH_NAMES) != 0, (want & MG_BATCH_PLACES) != 0, (want & MG_BATCH_EDITS) != 0,
                              (want & MG_BATCH_BASES) != 0);
}

int mg_bam_stream_file_named(const char* path, const mg_acc_index* ix, uint64_t chunk_bytes, int nthreads, mg_sam_batch** out,
                             int* err_kind, uint64_t* err_rec) {
  return bam_stream_file_impl(path, ix, chunk_bytes, nthreads, out, err_kind, err_rec, false, true);
}

int mg_bam_stream_file(const char* path, const mg_acc_index* ix, uint64_t chunk_bytes, int nthreads, mg_sam_batch** out,
                       int* err_kind, uint64_t* err_rec) {
  return bam_stream_file_impl(path, ix, chunk_bytes, nthreads, out, err_kind, err_rec, false);
}

int mg_bam_stream_file_collated(const char* path, const mg_acc_index* ix, uint64_t chunk_bytes, int nthreads, mg_sam_batch** out,
                                int* err_kind, uint64_t* err_rec) {
  return bam_stream_file_impl(path, ix, chunk_bytes, nthreads, out, err_kind, err_rec, true);
}

// What the file readers hand to the device for a plain FASTQ (kind 0) or SAM (kind 1) file, written to out_path instead: the
// pieces of `piece_bytes` slots thinned by nthreads readers, in order.  Host code only (no device, no mg_init): the thinning can be
// checked where there is no GPU.
int mg_stream_thin_file(const char* path, int kind, uint64_t piece_bytes, int nthreads, const char* out_path) {
  if (!path || !out_path) return fail(MG_ERR_ARG, "null argument");
  if (kind != 0 && kind != 1) return fail(MG_ERR_ARG, "kind must be 0 (fastq) or 1 (sam)");
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return fail(MG_ERR_ARG, "cannot open %s: %s", path, strerror(errno));
  struct stat sb;
  if (fstat(fd, &sb) != 0) { close(fd); return fail(MG_ERR_ARG, "cannot stat %s", path); }
  uint64_t cb = piece_bytes ? piece_bytes : (32ull << 20);
  if (cb < (1u << 16)) cb = 1u << 16;
  cb = (cb + 4095) & ~4095ull;
  ThinSource t;
  t.fd = fd;
  t.kind = kind == 0 ? ThinSource::kFastq : ThinSource::kSam;
  t.setup((uint64_t)sb.st_size, cb);
  std::vector<std::vector<uint8_t>> outs(t.npieces);
  std::atomic<uint64_t> next{0};
  std::atomic<bool> failed{false};
  auto work = [&]() {
    std::vector<uint8_t> buf(cb);
    for (;;) {
      const uint64_t i = next.fetch_add(1);
      if (i >= t.npieces) return;
      bool last = false;
      const int64_t n = t.fill(i, buf.data(), cb, &last);
      if (n < 0) { failed.store(true); return; }
      outs[i].assign(buf.begin(), buf.begin() + n);
    }
  };
  {
    if (nthreads < 1) nthreads = 1;
    std::vector<std::thread> th;
    for (int k = 1; k < nthreads; ++k) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
  }
  if (failed.load()) return fail(t.error_code, "%s", t.error.empty() ? "thinning failed" : t.error.c_str());
  FILE* fo = fopen(out_path, "wb");
  if (!fo) return fail(MG_ERR_ARG, "cannot open %s: %s", out_path, strerror(errno));
  bool ok = true;
  for (auto& o : outs) ok = ok && (o.empty() || fwrite(o.data(), 1, o.size(), fo) == o.size());
  ok = (fclose(fo) == 0) && ok;
  return ok ? MG_OK : fail(MG_ERR_ARG, "writing %s failed", out_path);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// organism files -> batches of genomes (mg_genomes_stream_*; `build_db --ingest device`)
// ---------------------------------------------------------------------------------------------------------------------
// Reader threads take WHOLE files in the order of the list (hundreds of thousands of them: parallelism across files is free) and
// leave each as a run of page-locked slabs — a plain file by positional reads, a ".gz" inflated by that thread with zlib, every
// member of it.  ONE uploader thread takes the slabs in file order and queues them on the copy stream into the text buffer of the
// batch it is filling (two buffers: batch i + 1 goes up while the caller parses and sketches batch i), closes the batch at a file
// boundary once it holds batch_bases bytes, and hands it to mg_genomes_stream_next, which parses it on the library stream.
// A slab goes to the reader of the file the uploader is waiting for, or to any reader while two are free: later files never
// starve the one everything waits for.  The text buffers are the uploader thread's own (hipMalloc: the pool is the caller
// thread's), so no block the main stream may still use is written on the copy stream; a buffer is written again only behind
// the event the main stream records after parsing its previous batch.
// Inflating these files ON THE DEVICE is not done: DevInflater takes one stream per call and does not tell which member ends
// belong to which file of a concatenation (DESIGN.md §8 f2').
struct mg_genomes_stream {
  struct Piece { int slab; uint64_t bytes; };
  struct FileQ { std::deque<Piece> pieces; bool done = false; };
  struct Batch { int buf = 0; const uint8_t* text = nullptr; std::vector<uint64_t> ext; uint64_t first = 0; };
  std::vector<std::string> paths;
  uint64_t batch_bases = 0, slab_bytes = 0;
  size_t nslots = 0;
  int device = 0;
  std::mutex m;
  std::condition_variable cv;
  // (under m)
  uint64_t next_file = 0, head = 0;  // the next file a reader takes; the file the uploader is at
  bool stop = false, failed = false, end = false;
  std::string error;
  std::vector<int> free_slabs;
  std::map<uint64_t, FileQ> active;
  std::deque<Batch> ready;
  uint64_t parsed = 0;  // batches whose parse has been queued on the library stream
  double read_s = 0, upload_s = 0, wait_s = 0, parse_s = 0;
  uint64_t text_bytes = 0;
  // (the uploader thread's)
  uint8_t* dtext[2] = {nullptr, nullptr};
  uint64_t cap[2] = {0, 0};
  std::vector<char> slab_used;  // (a slab's event has been recorded: under m with free_slabs)
  std::vector<std::thread> readers;
  std::thread uploader;
};

namespace mg {

using GS = mg_genomes_stream;
using Clock = std::chrono::steady_clock;
static double secs_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

static void gs_fail(GS* h, const std::string& msg) {
  std::lock_guard<std::mutex> lk(h->m);
  if (!h->failed) { h->failed = true; h->error = msg; }
  h->stop = true;
  h->cv.notify_all();
}

// a free slab for the reader of file i (-1: the stream stops); *waited += the seconds spent waiting for one
static int gs_acquire(GS* h, uint64_t i, double* waited) {
  int s = -1;
  bool used = false;
  const Clock::time_point t0 = Clock::now();
  struct Waited { double* w; Clock::time_point t0; ~Waited() { *w += secs_since(t0); } } add{waited, t0};
  {
    std::unique_lock<std::mutex> lk(h->m);
    h->cv.wait(lk, [&] { return h->stop || (!h->free_slabs.empty() && (i == h->head || h->free_slabs.size() >= 2)); });
    if (h->stop) return -1;
    s = h->free_slabs.back();
    h->free_slabs.pop_back();
    used = h->slab_used[s] != 0;
  }
  if (used) (void)hipEventSynchronize(g_res.ev_slot[s]);  // its last copy has left it
  return s;
}

static void gs_push(GS* h, uint64_t i, int slab, uint64_t bytes, bool done) {
  std::lock_guard<std::mutex> lk(h->m);
  GS::FileQ& q = h->active[i];
  if (slab >= 0) {
    if (bytes) q.pieces.push_back(GS::Piece{slab, bytes});
    else h->free_slabs.push_back(slab);
  }
  q.done = q.done || done;
  h->cv.notify_all();
}

// file i -> slabs; false = failed (the error is set) or stopped
static bool gs_read_file(GS* h, uint64_t i, std::vector<uint8_t>& in, double* waited) {
  const std::string& path = h->paths[i];
  const int fd = open(path.c_str(), O_RDONLY);
  if (fd < 0) { gs_fail(h, "cannot open " + path + ": " + strerror(errno)); return false; }
  struct Closer { int fd; ~Closer() { close(fd); } } closer{fd};
  const bool gz = path.size() >= 3 && path.compare(path.size() - 3, 3, ".gz") == 0;  // (what formats.read_sequences goes by)
  if (!gz) {
    struct stat sb;
    if (fstat(fd, &sb) != 0) { gs_fail(h, "cannot stat " + path + ": " + strerror(errno)); return false; }
    const uint64_t size = (uint64_t)sb.st_size;
    for (uint64_t at = 0; at < size;) {
      const int s = gs_acquire(h, i, waited);
      if (s < 0) return false;
      const uint64_t want = size - at < h->slab_bytes ? size - at : h->slab_bytes;
      uint64_t got = 0;
      while (got < want) {
        const ssize_t n = pread(fd, g_res.slots[s] + got, want - got, (off_t)(at + got));
        if (n < 0) { gs_fail(h, path + ": read failed: " + strerror(errno)); return false; }
        if (n == 0) { gs_fail(h, path + ": file is shorter than its size said"); return false; }
        got += (uint64_t)n;
      }
      at += want;
      gs_push(h, i, s, want, at >= size);
    }
    if (size == 0) gs_push(h, i, -1, 0, true);
    return true;
  }
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (inflateInit2(&zs, 15 + 16) != Z_OK) { gs_fail(h, path + ": inflateInit2 failed"); return false; }
  struct Ender { z_stream* z; ~Ender() { inflateEnd(z); } } ender{&zs};
  uint64_t in_off = 0;
  bool in_member = false, eof = false;  // between members only zero padding or another member may stand (Python's gzip module)
  while (!eof) {
    const int s = gs_acquire(h, i, waited);
    if (s < 0) return false;
    zs.next_out = g_res.slots[s];
    uint64_t room = h->slab_bytes;
    while (room > 0) {
      if (zs.avail_in == 0) {
        const ssize_t n = pread(fd, in.data(), in.size(), (off_t)in_off);
        if (n < 0) { gs_fail(h, path + ": read failed: " + strerror(errno)); return false; }
        if (n == 0) {
          if (in_member) { gs_fail(h, path + ": unexpected end of file (the gzip stream ends inside a member)"); return false; }
          eof = true;
          break;
        }
        in_off += (uint64_t)n;
        zs.next_in = in.data();
        zs.avail_in = (uInt)n;
      }
      if (!in_member) {
        while (zs.avail_in && zs.next_in[0] == 0) { ++zs.next_in; --zs.avail_in; }
        if (!zs.avail_in) continue;
        in_member = true;
      }
      zs.avail_out = (uInt)(room > 0x40000000ull ? 0x40000000ull : room);
      const uInt before = zs.avail_out;
      const int rc = inflate(&zs, Z_NO_FLUSH);
      room -= before - zs.avail_out;
      if (rc == Z_STREAM_END) {
        in_member = false;
        if (inflateReset(&zs) != Z_OK) { gs_fail(h, path + ": inflateReset failed"); return false; }
      } else if (rc != Z_OK && rc != Z_BUF_ERROR) {
        gs_fail(h, path + ": inflate failed: " + (zs.msg ? zs.msg : "corrupt gzip data"));
        return false;
      }
    }
    gs_push(h, i, s, h->slab_bytes - room, eof);
  }
  return true;
}

static void gs_reader(GS* h) {
  (void)hipSetDevice(h->device);
  std::vector<uint8_t> in(1u << 20);
  for (;;) {
    uint64_t i;
    {
      std::lock_guard<std::mutex> lk(h->m);
      if (h->stop || h->next_file >= h->paths.size()) return;
      i = h->next_file++;
    }
    const Clock::time_point t0 = Clock::now();
    double waited = 0;
    const bool ok = gs_read_file(h, i, in, &waited);
    {
      std::lock_guard<std::mutex> lk(h->m);
      h->read_s += secs_since(t0) - waited;  // (read + inflate: not the wait for a free slab)
    }
    if (!ok) return;
  }
}

static void gs_uploader(GS* h) {
  (void)hipSetDevice(h->device);
  StreamRes& r = g_res;
  const uint64_t nfiles = h->paths.size();
  auto hip_fail = [&](const char* what, hipError_t e) { gs_fail(h, std::string(what) + " failed: " + hipGetErrorString(e)); };
  for (uint64_t b = 0;; ++b) {
    const int buf = (int)(b & 1);
    {
      std::unique_lock<std::mutex> lk(h->m);
      h->cv.wait(lk, [&] { return h->stop || b < 2 || h->parsed + 2 > b; });  // the buffer's previous batch has been parsed
      if (h->stop) return;
      if (h->head >= nfiles) { h->end = true; h->cv.notify_all(); return; }
    }
    hipError_t e = hipSuccess;
    if (b >= 2 && (e = hipStreamWaitEvent(r.copy, r.ev_parsed[buf], 0)) != hipSuccess) { hip_fail("hipStreamWaitEvent", e); return; }
    GS::Batch batch;
    batch.buf = buf;
    batch.ext.push_back(0);
    uint64_t fill = 0;
    {
      std::lock_guard<std::mutex> lk(h->m);
      batch.first = h->head;
    }
    for (;;) {  // file by file
      bool file_done = false;
      while (!file_done) {
        GS::Piece pc{-1, 0};
        {
          std::unique_lock<std::mutex> lk(h->m);
          GS::FileQ* q = nullptr;
          h->cv.wait(lk, [&] {
            if (h->stop) return true;
            auto it = h->active.find(h->head);
            if (it == h->active.end()) return false;
            q = &it->second;
            return !q->pieces.empty() || q->done;
          });
          if (h->stop) return;
          if (!q->pieces.empty()) { pc = q->pieces.front(); q->pieces.pop_front(); }
          else file_done = true;
        }
        if (file_done) break;
        const Clock::time_point t0 = Clock::now();
        if (fill + pc.bytes + 16 > h->cap[buf]) {  // (a file that outgrows the batch's room: rare, and paid with a device-wide wait)
          uint64_t ncap = h->cap[buf] * 2;
          if (ncap < fill + pc.bytes + 16) ncap = fill + pc.bytes + 16;
          uint8_t* nt = nullptr;
          if ((e = hipMalloc(reinterpret_cast<void**>(&nt), ncap)) != hipSuccess) { hip_fail("hipMalloc of a text buffer", e); return; }
          if (fill) e = hipMemcpyAsync(nt, h->dtext[buf], fill, hipMemcpyDeviceToDevice, r.copy);
          if (e == hipSuccess) e = hipStreamSynchronize(r.copy);
          if (e != hipSuccess) { (void)hipFree(nt); hip_fail("growing a text buffer", e); return; }
          (void)hipFree(h->dtext[buf]);
          h->dtext[buf] = nt;
          h->cap[buf] = ncap;
        }
        e = hipMemcpyAsync(h->dtext[buf] + fill, r.slots[pc.slab], pc.bytes, hipMemcpyHostToDevice, r.copy);
        if (e == hipSuccess) e = hipEventRecord(r.ev_slot[pc.slab], r.copy);
        if (e != hipSuccess) { hip_fail("the copy of a slab", e); return; }
        fill += pc.bytes;
        {
          std::lock_guard<std::mutex> lk(h->m);
          h->slab_used[pc.slab] = 1;
          h->free_slabs.push_back(pc.slab);
          h->upload_s += secs_since(t0);
          h->text_bytes += pc.bytes;
          h->cv.notify_all();
        }
      }
      batch.ext.push_back(fill);
      bool close_batch;
      {
        std::lock_guard<std::mutex> lk(h->m);
        h->active.erase(h->head);
        ++h->head;
        close_batch = h->head >= nfiles || fill >= h->batch_bases;
        h->cv.notify_all();  // (the reader of the new head may take the last free slab)
      }
      if (close_batch) break;
    }
    if ((e = hipEventRecord(r.ev_h2d[buf], r.copy)) != hipSuccess) { hip_fail("hipEventRecord", e); return; }
    batch.text = h->dtext[buf];
    {
      std::lock_guard<std::mutex> lk(h->m);
      h->ready.push_back(std::move(batch));
      h->cv.notify_all();
    }
  }
}

}  // namespace mg

extern "C" {

void mg_genomes_stream_close(mg_genomes_stream* h) {
  if (!h) return;
  {
    std::lock_guard<std::mutex> lk(h->m);
    h->stop = true;
    h->cv.notify_all();
  }
  for (auto& t : h->readers) if (t.joinable()) t.join();
  if (h->uploader.joinable()) h->uploader.join();
  if (g_res.copy) (void)hipStreamSynchronize(g_res.copy);
  if (ctx().ready) (void)hipStreamSynchronize(ctx().stream);  // (a parse may still read the text)
  for (int b = 0; b < 2; ++b) if (h->dtext[b]) (void)hipFree(h->dtext[b]);
  delete h;
}

int mg_genomes_stream_open(const char* const* paths, uint64_t nfiles, uint64_t batch_bases, int nthreads, mg_genomes_stream** out) {
  MG_REQUIRE_READY();
  if (!out) return fail(MG_ERR_ARG, "null out handle");
  *out = nullptr;
  if (nfiles && !paths) return fail(MG_ERR_ARG, "null paths");
  for (uint64_t i = 0; i < nfiles; ++i) if (!paths[i]) return fail(MG_ERR_ARG, "null path");
  if (nthreads <= 0 || nthreads > 16) nthreads = 16;  // (never by the machine's core count)
  if ((uint64_t)nthreads > nfiles) nthreads = nfiles ? (int)nfiles : 1;
  uint64_t slab = dbg("genome_slab_bytes") > 0 ? (uint64_t)dbg("genome_slab_bytes") : (8ull << 20);
  if (slab < 4096) slab = 4096;
  slab = (slab + 4095) & ~4095ull;
  std::unique_ptr<mg_genomes_stream, void (*)(mg_genomes_stream*)> h(new mg_genomes_stream(), mg_genomes_stream_close);
  h->paths.assign(paths, paths + nfiles);
  h->batch_bases = batch_bases ? batch_bases : (1ull << 27);
  h->slab_bytes = slab;
  h->nslots = (size_t)nthreads + 2;
  h->device = ctx().device;
  MG_TRY(ensure_res(slab, h->nslots));
  MG_HIP(hipStreamSynchronize(g_res.copy));  // (slots and events of an earlier streaming call)
  h->slab_used.assign(h->nslots, 0);
  for (size_t s = 0; s < h->nslots; ++s) h->free_slabs.push_back((int)s);
  for (int b = 0; b < 2; ++b) {
    h->cap[b] = h->batch_bases + slab + 16;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->dtext[b]), h->cap[b]);
    if (e != hipSuccess) return fail(MG_ERR_NOMEM, "hipMalloc(%llu) of a text buffer failed: %s", (unsigned long long)h->cap[b], hipGetErrorString(e));
  }
  mg_genomes_stream* raw = h.get();
  for (int t = 0; t < nthreads; ++t) raw->readers.emplace_back(gs_reader, raw);
  raw->uploader = std::thread(gs_uploader, raw);
  *out = h.release();
  return MG_OK;
}

int mg_genomes_stream_next(mg_genomes_stream* h, mg_genomes** batch, uint64_t* first_file, uint64_t* nfiles_in_batch,
                           uint8_t* undecided_flags) {
  MG_REQUIRE_READY();
  if (!h || !batch || !first_file || !nfiles_in_batch) return fail(MG_ERR_ARG, "null argument");
  *batch = nullptr;
  *nfiles_in_batch = 0;
  *first_file = h->paths.size();
  mg_genomes_stream::Batch b;
  {
    const Clock::time_point t0 = Clock::now();
    std::unique_lock<std::mutex> lk(h->m);
    h->cv.wait(lk, [&] { return h->failed || !h->ready.empty() || h->end; });
    h->wait_s += secs_since(t0);
    if (h->failed) return fail(MG_ERR_ARG, "%s", h->error.c_str());
    if (h->ready.empty()) return MG_OK;  // after the last file
    b = std::move(h->ready.front());
    h->ready.pop_front();
  }
  const Clock::time_point t0 = Clock::now();
  hipStream_t st = ctx().stream;
  int rc = hipStreamWaitEvent(st, g_res.ev_h2d[b.buf], 0) == hipSuccess ? MG_OK : fail(MG_ERR_HIP, "hipStreamWaitEvent failed");
  const uint64_t nf = b.ext.size() - 1;
  if (rc == MG_OK) rc = mg_genomes_parse_dev(b.text, b.ext.data(), nf, batch, undecided_flags);
  if (hipEventRecord(g_res.ev_parsed[b.buf], st) != hipSuccess && rc == MG_OK) rc = fail(MG_ERR_HIP, "hipEventRecord failed");
  {
    std::lock_guard<std::mutex> lk(h->m);
    ++h->parsed;
    h->parse_s += secs_since(t0);
    h->cv.notify_all();
  }
  if (rc != MG_OK) { mg_genomes_free(*batch); *batch = nullptr; return rc; }
  *first_file = b.first;
  *nfiles_in_batch = nf;
  return MG_OK;
}

int mg_genomes_stream_stats(const mg_genomes_stream* h, double out[5]) {
  if (!h || !out) return fail(MG_ERR_ARG, "null argument");
  mg_genomes_stream* w = const_cast<mg_genomes_stream*>(h);
  std::lock_guard<std::mutex> lk(w->m);
  out[0] = h->read_s; out[1] = h->upload_s; out[2] = h->wait_s; out[3] = h->parse_s; out[4] = (double)h->text_bytes;
  return MG_OK;
}

}  // extern "C"
