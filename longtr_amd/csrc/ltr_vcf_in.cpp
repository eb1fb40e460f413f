// ltr_vcf_in.cpp -- tabix-indexed VCF input without htslib (--ref-vcf): a BGZF VCF with its .tbi, read through the
// shared BGZF reader and binning index of ltr_bgzf.h, and the writer of such an index.  Host code; citations are to
// the LongTR reference:
//   VCFReader::open                       src/vcf_reader.cpp:74-105 (its error messages; tbx_index_load, tbx_seqnames)
//   VCFReader::set_region / get_next_variant   src/vcf_reader.h:215-227, src/vcf_reader.cpp:114-120 (tbx_itr_querys + tbx_itr_next)
//   read_vcf_alleles                      src/vcf_input.cpp:21-50
// The tabix index is the BAI binning + linear index behind a header of its own (magic "TBI\1", n_ref, format, col_seq,
// col_beg, col_end, meta, skip, l_nm, names), the whole file BGZF-compressed.  A record's interval is
// [POS-1, max(POS-1+len(REF), INFO END)): the one ltr_vcf_index writes into the bins and the one a query tests.
// Not here: .csi indexes, plain-text VCFs, the header's ##INFO typing (INFO values are read as text).

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include <sys/stat.h>
#include <zlib.h>

#include "ltr_bgzf.h"
#include "ltr_internal.h"

namespace {

namespace bgzf = ltr::bgzf;
using bgzf::Chunk;

constexpr int32_t kPad = 50;                      // read_vcf_alleles' window either side of the region (vcf_input.cpp:18)

void put_error(char* err, int cap, const std::string& msg) {
  if (!err || cap <= 0) return;
  const size_t n = std::min(msg.size(), (size_t)cap - 1);
  std::memcpy(err, msg.data(), n);
  err[n] = 0;
}

struct TbiRef { std::map<uint32_t, std::vector<Chunk>> bins; std::vector<uint64_t> linear; int64_t n_chunks = 0; };
struct Tbi {
  int32_t format = 0, col_seq = 0, col_beg = 0, col_end = 0, meta = 0, skip = 0;
  std::vector<std::string> names;
  std::vector<TbiRef> refs;
};

// The whole decompressed content of a BGZF file; false when it is not one or a block is damaged.
bool read_all(const std::string& path, std::vector<uint8_t>* out) {
  bgzf::Reader z;
  z.f = std::fopen(path.c_str(), "rb");
  if (!z.f) return false;
  int64_t addr = 0;
  while (z.load(addr)) { out->insert(out->end(), z.data.begin(), z.data.end()); addr = z.next_addr; }
  return !z.bad && addr > 0;
}

// The tabix index (htslib's tbx_index_load layout).  Chunks of the metadata pseudo-bin are not kept (its second
// "chunk" holds record counts); every other chunk must have beg <= end.
bool parse_tbi(const std::vector<uint8_t>& b, Tbi* t) {
  size_t at = 0;
  auto need = [&](size_t k) { return at + k <= b.size(); };
  auto i32 = [&]() { const int32_t v = (int32_t)bgzf::le32(b.data() + at); at += 4; return v; };
  if (!need(36) || std::memcmp(b.data(), "TBI\1", 4) != 0) return false;
  at = 4;
  const int32_t n_ref = i32();
  t->format = i32(); t->col_seq = i32(); t->col_beg = i32(); t->col_end = i32(); t->meta = i32(); t->skip = i32();
  const int32_t l_nm = i32();
  if (n_ref < 0 || l_nm < 0 || !need((size_t)l_nm) || (size_t)n_ref * 8 > b.size()) return false;
  for (size_t k = at, e = at + (size_t)l_nm; k < e;) {
    const uint8_t* z = (const uint8_t*)std::memchr(b.data() + k, 0, e - k);
    if (!z) return false;
    t->names.emplace_back((const char*)b.data() + k, (size_t)(z - (b.data() + k)));
    k = (size_t)(z - b.data()) + 1;
  }
  at += (size_t)l_nm;
  if ((int32_t)t->names.size() != n_ref) return false;
  t->refs.resize((size_t)n_ref);
  for (int32_t r = 0; r < n_ref; ++r) {
    TbiRef& R = t->refs[(size_t)r];
    if (!need(4)) return false;
    const int32_t n_bin = i32();
    if (n_bin < 0) return false;
    for (int32_t k = 0; k < n_bin; ++k) {
      if (!need(8)) return false;
      const uint32_t bin = bgzf::le32(b.data() + at); at += 4;
      const int32_t n_chunk = i32();
      if (n_chunk < 0 || !need((size_t)n_chunk * 16)) return false;
      std::vector<Chunk> ch((size_t)n_chunk);
      for (int32_t c = 0; c < n_chunk; ++c, at += 16) ch[(size_t)c] = {bgzf::le64(b.data() + at), bgzf::le64(b.data() + at + 8)};
      if (bin == bgzf::kMetaBin) continue;
      for (const Chunk& c : ch) if (c.beg > c.end) return false;
      R.n_chunks += n_chunk;
      std::vector<Chunk>& dst = R.bins[bin];
      dst.insert(dst.end(), ch.begin(), ch.end());
    }
    if (!need(4)) return false;
    const int32_t n_intv = i32();
    if (n_intv < 0 || !need((size_t)n_intv * 8)) return false;
    R.linear.resize((size_t)n_intv);
    for (int32_t k = 0; k < n_intv; ++k, at += 8) R.linear[(size_t)k] = bgzf::le64(b.data() + at);
  }
  return true;                                    // (an optional n_no_coor may follow)
}

// One text line of a BGZF stream, without its '\n': 1 = a line, 0 = end of file, < 0 = damaged file.
int read_line(bgzf::Reader& z, std::string* line) {
  line->clear();
  for (;;) {
    if (z.block_addr < 0 || z.at >= z.data.size()) {
      bool ok;
      do { ok = z.load(z.block_addr < 0 ? 0 : z.next_addr); } while (ok && z.data.empty());   // (empty blocks: the end-of-file marker)
      if (!ok) return z.bad ? LTR_ERR_INVALID : (line->empty() ? 0 : 1);
    }
    const char* b = (const char*)z.data.data() + z.at;
    const size_t avail = z.data.size() - z.at;
    const char* nl = (const char*)std::memchr(b, '\n', avail);
    if (nl) { line->append(b, (size_t)(nl - b)); z.at += (size_t)(nl - b) + 1; return 1; }
    line->append(b, avail); z.at = z.data.size();
  }
}

// The INFO value of `key` as one integer: 1 = read, 0 = no such key, -1 = present but not a single integer (where
// the reference's get_INFO_value_single_int ends the process, vcf_reader.h:112-118).
int info_int(const std::string& info, const char* key, int64_t* value) {
  const size_t kl = std::strlen(key);
  size_t k = 0;
  while (k <= info.size()) {
    size_t e = info.find(';', k);
    if (e == std::string::npos) e = info.size();
    if (e - k >= kl && info.compare(k, kl, key) == 0 && (e - k == kl || info[k + kl] == '=')) {
      if (e - k <= kl + 1) return -1;
      const std::string v = info.substr(k + kl + 1, e - k - kl - 1);
      char* endp = nullptr;
      const long long x = std::strtoll(v.c_str(), &endp, 10);
      if (*endp || x < INT32_MIN || x > INT32_MAX) return -1;
      *value = x;
      return 1;
    }
    k = e + 1;
  }
  return 0;
}

// The columns of a data line a query and read_vcf_alleles need.
struct VcfLine {
  std::string chrom, ref, alt, info;
  int64_t pos = 0;                                // POS (1-based)
  int64_t beg = 0, end = 0;                       // the record's interval, 0-based half open
};

// false: fewer than 8 columns or an unreadable POS
bool split_line(const std::string& s, VcfLine* v) {
  size_t col[8], n = 0, k = 0;
  col[n++] = 0;
  while (n < 8 && (k = s.find('\t', k)) != std::string::npos) col[n++] = ++k;
  if (n < 8) return false;
  auto field = [&](int i) {
    const size_t e = (i + 1 < 8) ? col[i + 1] - 1 : std::min(s.find('\t', col[7]), s.size());
    return s.substr(col[i], e - col[i]);
  };
  v->chrom = field(0);
  const std::string p = field(1);
  char* endp = nullptr;
  v->pos = std::strtoll(p.c_str(), &endp, 10);
  if (p.empty() || *endp || v->pos < 1 || v->pos > (1 << 29)) return false;
  v->ref = field(3); v->alt = field(4); v->info = field(7);
  v->beg = v->pos - 1;
  v->end = v->beg + (int64_t)std::max<size_t>(v->ref.size(), 1);
  int64_t end_info = 0;
  if (info_int(v->info, "END", &end_info) == 1) v->end = std::max(v->end, end_info);
  return true;
}

}  // namespace

struct ltr_vcf_reader {
  std::string path;
  bgzf::Reader z;
  Tbi tbi;
  std::map<std::string, int32_t> ids;
};

namespace {

// tbx_itr_querys + tbx_itr_next: the records whose interval overlaps [beg, end), in file order, handed to f until it
// returns false.  1 = the chromosome is indexed, 0 = it is not (the reference's set_region fails), < 0 = damaged file.
template <class F>
int query(ltr_vcf_reader* r, const std::string& chrom, int64_t beg, int64_t end, F&& f) {
  auto it = r->ids.find(chrom);
  if (it == r->ids.end()) return 0;
  beg = std::max<int64_t>(beg, 0);
  if (end <= beg) return 1;
  const TbiRef& ix = r->tbi.refs[(size_t)it->second];
  const std::vector<Chunk> todo = bgzf::query_chunks(ix.bins, ix.linear, beg, end);
  r->z.bad = false;                               // (a damaged block met by an earlier query does not poison this one)
  std::string line;
  VcfLine v;
  for (const Chunk& c : todo) {
    if (!r->z.seek(c.beg)) return LTR_ERR_INVALID;
    while (r->z.tell() < c.end) {
      const int rc = read_line(r->z, &line);
      if (rc < 0) return rc;
      if (rc == 0) break;
      if (line.empty() || line[0] == (char)r->tbi.meta) continue;
      if (!split_line(line, &v)) return LTR_ERR_INVALID;
      if (v.chrom != chrom || v.beg >= end) return 1;      // position-sorted: nothing further can overlap
      if (v.end > beg && !f(v, line)) return 1;
    }
  }
  return 1;
}

}  // namespace

extern "C" {

// VCFReader::open (vcf_reader.cpp:74-105) without the htslib header parse: the file must be BGZF, its index
// <path>.tbi no older than it, and the text must start like a VCF.
int ltr_vcf_reader_open(const char* path, ltr_vcf_reader** out, char* err, int err_cap) {
  if (!path || !out) return LTR_ERR_INVALID;
  *out = nullptr;
  try {
    std::unique_ptr<ltr_vcf_reader> r(new ltr_vcf_reader());
    r->path = path;
    const std::string tbi = r->path + ".tbi";
    struct stat st_vcf, st_tbi;
    if (stat(path, &st_vcf) != 0 || !(r->z.f = std::fopen(path, "rb"))) { put_error(err, err_cap, "Failed to open the VCF file " + r->path); return LTR_ERR_INVALID; }
    if (stat(tbi.c_str(), &st_tbi) == 0 && st_vcf.st_mtime > st_tbi.st_mtime) {
      put_error(err, err_cap, "The tabix index for the VCF file is older than the VCF itself. Please reindex the VCF with tabix");
      return LTR_ERR_INVALID;
    }
    if (!r->z.load(0)) { put_error(err, err_cap, "VCF file is not bgzipped. Please ensure bgzip was used to compress it"); return LTR_ERR_INVALID; }
    std::vector<uint8_t> bytes;
    if (!read_all(tbi, &bytes) || !parse_tbi(bytes, &r->tbi)) { put_error(err, err_cap, "Failed to open the VCF file's tabix index " + tbi); return LTR_ERR_INVALID; }
    if (r->tbi.names.empty()) { put_error(err, err_cap, "VCF does not contain any chromosomes"); return LTR_ERR_INVALID; }
    for (size_t i = 0; i < r->tbi.names.size(); ++i) r->ids[r->tbi.names[i]] = (int32_t)i;
    // the header: meta lines, then the #CHROM line; nothing of it is kept
    std::string line;
    bool first = true, chrom_line = false;
    while (!chrom_line) {
      const int rc = read_line(r->z, &line);
      if (rc <= 0 || line.empty() || line[0] != '#' || (first && line.compare(0, 16, "##fileformat=VCF") != 0)) {
        put_error(err, err_cap, "Provided VCF file is improperly formatted");
        return LTR_ERR_INVALID;
      }
      first = false;
      chrom_line = line.compare(0, 6, "#CHROM") == 0;
    }
    *out = r.release();
    return LTR_OK;
  } catch (const std::bad_alloc&) { put_error(err, err_cap, "out of host memory"); return LTR_ERR_NOMEM; }
  catch (const std::exception& e) { put_error(err, err_cap, std::string("internal error: ") + e.what()); return LTR_ERR_INVALID; }
}

void ltr_vcf_reader_close(ltr_vcf_reader* r) { delete r; }

// read_vcf_alleles (vcf_input.cpp:21-50): the record of the window [max(0, start-50), stop+50) whose INFO START / END
// are region_start+1 / region_stop; records without both are skipped, the scan ends after the first record past
// region_start+50.  1 = found (*pos = POS-1, the alleles REF first, then the ALTs in file order), 0 = not found
// (*pos = -1), < 0 = a malformed record or too small a buffer.
int ltr_vcf_read_alleles(ltr_vcf_reader* r, const char* chrom, int32_t region_start, int32_t region_stop, int32_t* pos,
                         char* out, int64_t cap, int64_t* allele_off, int32_t* n_alleles) {
  if (!r || !chrom || !pos || !out || !allele_off || !n_alleles || cap < 0) return LTR_ERR_INVALID;
  *pos = -1; *n_alleles = 0;
  try {
    const int64_t pad_start = region_start < kPad ? 0 : (int64_t)region_start - kPad;
    int status = 0;
    const int rc = query(r, chrom, pad_start, (int64_t)region_stop + kPad, [&](const VcfLine& v, const std::string&) {
      int64_t start = 0, stop = 0;
      const int a = info_int(v.info, "START", &start), b = info_int(v.info, "END", &stop);
      if (a < 0 || b < 0) { status = LTR_ERR_INVALID; return false; }
      if (a == 1 && b == 1) {
        if (start == (int64_t)region_start + 1 && stop == region_stop) {
          std::vector<std::string> alleles{v.ref};
          if (v.alt != ".") {
            size_t k = 0;
            for (;;) {
              const size_t e = v.alt.find(',', k);
              alleles.push_back(v.alt.substr(k, e == std::string::npos ? std::string::npos : e - k));
              if (e == std::string::npos) break;
              k = e + 1;
            }
          }
          int64_t at = 0;
          allele_off[0] = 0;
          for (size_t i = 0; i < alleles.size(); ++i) {
            if (alleles[i].empty() || at + (int64_t)alleles[i].size() > cap) { status = LTR_ERR_INVALID; return false; }
            std::memcpy(out + at, alleles[i].data(), alleles[i].size());
            at += (int64_t)alleles[i].size();
            allele_off[i + 1] = at;
          }
          *n_alleles = (int32_t)alleles.size();
          *pos = (int32_t)(v.pos - 1);
          status = 1;
          return false;
        }
      }
      return v.pos <= (int64_t)region_start + kPad;
    });
    if (rc < 0) return rc;
    if (status != 1) { *pos = -1; *n_alleles = 0; }
    return status;
  } catch (const std::bad_alloc&) { return LTR_ERR_NOMEM; } catch (...) { return LTR_ERR_INVALID; }
}

// tabix -p vcf: <path>.tbi for a position-sorted BGZF VCF.  Records are binned by [POS-1, max(POS-1+len(REF), END));
// chunks of consecutive records in one bin are merged; the linear index holds, per 16 kb window, the offset of the
// first record that overlaps it (empty windows take the offset of the window before).
int ltr_vcf_index(const char* path) {
  if (!path) return LTR_ERR_INVALID;
  try {
    bgzf::Reader z;
    if (!(z.f = std::fopen(path, "rb")) || !z.load(0)) return LTR_ERR_INVALID;
    const uint64_t kUnset = ~0ull;
    std::vector<std::string> names;
    std::map<std::string, int32_t> ids;
    std::vector<std::map<uint32_t, std::vector<Chunk>>> bins;
    std::vector<std::vector<uint64_t>> linear;
    int32_t cur = -1; int64_t last_beg = -1;
    std::string line;
    VcfLine v;
    for (;;) {
      const uint64_t off0 = z.tell();
      const int rc = read_line(z, &line);
      if (rc < 0) return rc;
      if (rc == 0) break;
      if (line.empty() || line[0] == '#') continue;
      const uint64_t off1 = z.tell();
      if (!split_line(line, &v) || v.end > (int64_t)1 << 29) return LTR_ERR_INVALID;
      auto it = ids.find(v.chrom);
      if (it == ids.end()) {
        it = ids.emplace(v.chrom, (int32_t)names.size()).first;
        names.push_back(v.chrom); bins.emplace_back(); linear.emplace_back();
      } else if (it->second != cur || v.beg < last_beg) {
        return LTR_ERR_INVALID;                   // not sorted by chromosome and position
      }
      cur = it->second; last_beg = v.beg;
      std::vector<Chunk>& ch = bins[(size_t)cur][bgzf::reg2bin(v.beg, v.end)];
      if (!ch.empty() && ch.back().end == off0) ch.back().end = off1;
      else ch.push_back({off0, off1});
      std::vector<uint64_t>& lin = linear[(size_t)cur];
      const size_t w1 = (size_t)((v.end - 1) >> bgzf::kLinearShift);
      if (lin.size() <= w1) lin.resize(w1 + 1, kUnset);
      for (size_t w = (size_t)(v.beg >> bgzf::kLinearShift); w <= w1; ++w) if (lin[w] == kUnset) lin[w] = off0;
    }
    std::vector<uint8_t> b;
    auto put32 = [&](uint32_t x) { for (int k = 0; k < 4; ++k) b.push_back((uint8_t)(x >> (8 * k))); };
    auto put64 = [&](uint64_t x) { put32((uint32_t)x); put32((uint32_t)(x >> 32)); };
    b.insert(b.end(), {'T', 'B', 'I', 1});
    std::string nm;
    for (const std::string& n : names) { nm += n; nm.push_back('\0'); }
    put32((uint32_t)names.size());
    put32(2); put32(1); put32(2); put32(0); put32('#'); put32(0);   // TBX_VCF preset: format, col_seq / beg / end, meta, skip
    put32((uint32_t)nm.size());
    b.insert(b.end(), nm.begin(), nm.end());
    for (size_t r = 0; r < names.size(); ++r) {
      put32((uint32_t)bins[r].size());
      for (const auto& kv : bins[r]) {
        put32(kv.first); put32((uint32_t)kv.second.size());
        for (const Chunk& c : kv.second) { put64(c.beg); put64(c.end); }
      }
      std::vector<uint64_t>& lin = linear[r];
      for (size_t w = 0; w < lin.size(); ++w) if (lin[w] == kUnset) lin[w] = w ? lin[w - 1] : 0;
      put32((uint32_t)lin.size());
      for (uint64_t o : lin) put64(o);
    }
    const std::string tbi = std::string(path) + ".tbi";
    FILE* f = std::fopen(tbi.c_str(), "wb");
    if (!f) return LTR_ERR_INVALID;
    bool ok = true;
    for (size_t done = 0; ok && done < b.size(); done += bgzf::kBlock) ok = bgzf::write_block(f, b.data() + done, std::min(bgzf::kBlock, b.size() - done));
    ok = ok && std::fwrite(bgzf::kEof, 1, sizeof(bgzf::kEof), f) == sizeof(bgzf::kEof);
    ok = (std::fclose(f) == 0) && ok;
    return ok ? LTR_OK : LTR_ERR_INVALID;
  } catch (const std::bad_alloc&) { return LTR_ERR_NOMEM; } catch (...) { return LTR_ERR_INVALID; }
}

// Test hook: the lines of the records whose interval overlaps [start, end), each followed by '\n'.  Returns their
// length (0 for an unknown chromosome) or < 0 (damaged file, cap too small).
int64_t ltr_debug_vcf_query(ltr_vcf_reader* r, const char* chrom, int64_t start, int64_t end, char* out, int64_t cap) {
  if (!r || !chrom || (!out && cap > 0)) return LTR_ERR_INVALID;
  try {
    int64_t at = 0;
    bool room = true;
    const int rc = query(r, chrom, start, end, [&](const VcfLine&, const std::string& line) {
      if (at + (int64_t)line.size() + 1 > cap) { room = false; return false; }
      std::memcpy(out + at, line.data(), line.size());
      at += (int64_t)line.size();
      out[at++] = '\n';
      return true;
    });
    if (rc < 0) return rc;
    return room ? at : LTR_ERR_INVALID;
  } catch (const std::bad_alloc&) { return LTR_ERR_NOMEM; } catch (...) { return LTR_ERR_INVALID; }
}

// Test hook: parse a .tbi on its own.  header[6] = format, col_seq, col_beg, col_end, meta, skip; counts[2 r], counts[2 r + 1]
// = bins and chunks of reference r (metadata pseudo-bin excluded) for r < cap_refs; names = the NUL-terminated names back to
// back.  Returns the number of references, or LTR_ERR_INVALID for a file that is not a readable index (a chunk with
// beg > end included).
int32_t ltr_debug_tbi_parse(const char* tbi_path, int32_t* header, int64_t* counts, int32_t cap_refs, char* names, int64_t names_cap) {
  if (!tbi_path || !header) return LTR_ERR_INVALID;
  try {
    std::vector<uint8_t> bytes;
    Tbi t;
    if (!read_all(tbi_path, &bytes) || !parse_tbi(bytes, &t)) return LTR_ERR_INVALID;
    const int32_t h[6] = {t.format, t.col_seq, t.col_beg, t.col_end, t.meta, t.skip};
    std::memcpy(header, h, sizeof(h));
    for (size_t r = 0; counts && r < t.refs.size() && (int32_t)r < cap_refs; ++r) {
      counts[2 * r] = (int64_t)t.refs[r].bins.size();
      counts[2 * r + 1] = t.refs[r].n_chunks;
    }
    int64_t at = 0;
    for (const std::string& n : t.names) {
      if (!names || at + (int64_t)n.size() + 1 > names_cap) break;
      std::memcpy(names + at, n.c_str(), n.size() + 1);
      at += (int64_t)n.size() + 1;
    }
    return (int32_t)t.refs.size();
  } catch (const std::bad_alloc&) { return LTR_ERR_NOMEM; } catch (...) { return LTR_ERR_INVALID; }
}

}  // extern "C"
