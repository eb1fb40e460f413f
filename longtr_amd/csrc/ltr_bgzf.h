// ltr_bgzf.h -- internal: the BGZF container and the binning index shared by the htslib-free readers and writers
// (ltr_bam.cpp: BAM + BAI, ltr_vcf_in.cpp: VCF + TBI, ltr_io.cpp: the BGZF VCF writer).  BGZF = gzip members of
// <= 64 KB with a 'BC' extra field holding the member's size, addressed by virtual offsets (coffset << 16 | uoffset);
// the binning scheme is the one of the SAM specification (sections 4.1, 5.1-5.3), which tabix shares.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <sys/types.h>
#include <zlib.h>

namespace ltr {
namespace bgzf {

inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint64_t le64(const uint8_t* p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }
inline uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }

// ---- reader: one inflated block at a time, addressed by virtual offsets ----
struct Reader {
  FILE* f = nullptr;
  int64_t block_addr = -1, next_addr = 0;         // file offset of the block in `data` / of the one after it
  std::vector<uint8_t> data;                      // inflated bytes of the current block
  size_t at = 0;
  bool bad = false;
  ~Reader() { if (f) std::fclose(f); }
  bool load(int64_t addr) {                       // false: end of file or a damaged block (bad)
    uint8_t head[18];
    if (fseeko(f, (off_t)addr, SEEK_SET) != 0) { bad = true; return false; }
    const size_t got = std::fread(head, 1, 18, f);
    if (got == 0) return false;
    if (got != 18 || head[0] != 0x1f || head[1] != 0x8b || head[2] != 8 || !(head[3] & 4)) { bad = true; return false; }
    // the extra field holds the BC subfield (possibly after others)
    const int xlen = le16(head + 10);
    std::vector<uint8_t> extra((size_t)xlen);
    std::memcpy(extra.data(), head + 12, std::min<size_t>(6, (size_t)xlen));
    if (xlen > 6 && std::fread(extra.data() + 6, 1, (size_t)xlen - 6, f) != (size_t)xlen - 6) { bad = true; return false; }
    int bsize = -1;
    for (int k = 0; k + 4 <= xlen;) {
      const int slen = le16(extra.data() + k + 2);
      if (extra[(size_t)k] == 'B' && extra[(size_t)k + 1] == 'C' && slen == 2 && k + 6 <= xlen) bsize = le16(extra.data() + k + 4) + 1;
      k += 4 + slen;
    }
    if (bsize < 12 + xlen + 8) { bad = true; return false; }
    const size_t clen = (size_t)bsize - 12 - (size_t)xlen - 8;
    std::vector<uint8_t> comp(clen + 8);
    if (std::fread(comp.data(), 1, clen + 8, f) != clen + 8) { bad = true; return false; }
    const uint32_t isize = le32(comp.data() + clen + 4);
    if (isize > 65536) { bad = true; return false; }
    // (inflated into a buffer of its own and committed only once the block is whole: a damaged block never replaces --
    // or half-overwrites -- the bytes block_addr stands for)
    std::vector<uint8_t> fresh(isize);
    if (isize) {
      z_stream zs; std::memset(&zs, 0, sizeof(zs));
      if (inflateInit2(&zs, -15) != Z_OK) { bad = true; return false; }
      zs.next_in = comp.data(); zs.avail_in = (uInt)clen; zs.next_out = fresh.data(); zs.avail_out = isize;
      const int rc = inflate(&zs, Z_FINISH);
      inflateEnd(&zs);
      if (rc != Z_STREAM_END || zs.total_out != isize || (uint32_t)crc32(crc32(0L, Z_NULL, 0), fresh.data(), isize) != le32(comp.data() + clen)) { bad = true; return false; }
    }
    data.swap(fresh);
    block_addr = addr; next_addr = addr + bsize; at = 0;
    return true;
  }
  bool seek(uint64_t voff) {
    const int64_t addr = (int64_t)(voff >> 16);
    if (addr != block_addr && !load(addr)) return false;
    at = (size_t)(voff & 0xffff);
    return at <= data.size();
  }
  uint64_t tell() const { return at < data.size() || block_addr < 0 ? (((uint64_t)block_addr) << 16) | at : ((uint64_t)next_addr) << 16; }
  bool read(void* dst, size_t n) {                // false: fewer than n bytes left (end of file when !bad and nothing was read)
    uint8_t* out = (uint8_t*)dst;
    while (n) {
      if (block_addr < 0 || at >= data.size()) {
        do { if (!load(block_addr < 0 ? 0 : next_addr)) return false; } while (data.empty());    // (empty blocks: the end-of-file marker)
      }
      const size_t k = std::min(n, data.size() - at);
      std::memcpy(out, data.data() + at, k);
      out += k; at += k; n -= k;
    }
    return true;
  }
};

// ---- writer: one member per call ----
constexpr size_t kBlock = 0xff00;                 // uncompressed bytes per block (htslib's BGZF_BLOCK_SIZE)
const uint8_t kEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

inline bool write_block(FILE* f, const uint8_t* data, size_t n) {
  uint8_t out[0x10000];
  z_stream zs; std::memset(&zs, 0, sizeof(zs));
  if (deflateInit2(&zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
  zs.next_in = const_cast<uint8_t*>(data); zs.avail_in = (uInt)n;
  zs.next_out = out + 18; zs.avail_out = sizeof(out) - 18 - 8;
  const int rc = deflate(&zs, Z_FINISH);
  const size_t clen = zs.total_out;
  deflateEnd(&zs);
  if (rc != Z_STREAM_END) return false;                         // (0xff00 bytes always fit: deflate's worst case adds 5 bytes per 16 KB)
  const size_t total = 18 + clen + 8;
  const uint8_t head[18] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0,
                            (uint8_t)((total - 1) & 0xff), (uint8_t)((total - 1) >> 8)};
  std::memcpy(out, head, 18);
  const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), data, (uInt)n);
  uint8_t* tail = out + 18 + clen;
  for (int k = 0; k < 4; ++k) { tail[k] = (uint8_t)(crc >> (8 * k)); tail[4 + k] = (uint8_t)((uint32_t)n >> (8 * k)); }
  return std::fwrite(out, 1, total, f) == total;
}

// ---- binning index (SAM specification 5.1-5.3; BAI and TBI share it) ----
struct Chunk { uint64_t beg, end; };
constexpr uint32_t kMetaBin = 37450;              // the pseudo-bin of per-reference metadata
constexpr int kLinearShift = 14;                  // 16 kb windows of the linear index

// reg2bins: the bins a region [beg, end) can overlap
inline void reg2bins(int64_t beg, int64_t end, std::vector<uint32_t>& bins) {
  --end;
  bins.push_back(0);
  for (int64_t k = 1 + (beg >> 26); k <= 1 + (end >> 26); ++k) bins.push_back((uint32_t)k);
  for (int64_t k = 9 + (beg >> 23); k <= 9 + (end >> 23); ++k) bins.push_back((uint32_t)k);
  for (int64_t k = 73 + (beg >> 20); k <= 73 + (end >> 20); ++k) bins.push_back((uint32_t)k);
  for (int64_t k = 585 + (beg >> 17); k <= 585 + (end >> 17); ++k) bins.push_back((uint32_t)k);
  for (int64_t k = 4681 + (beg >> 14); k <= 4681 + (end >> 14); ++k) bins.push_back((uint32_t)k);
}

// reg2bin: the smallest bin that holds all of [beg, end)
inline uint32_t reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}

// The chunks of one reference that a query of [beg, end) has to read, in file order with overlaps merged:
// every chunk of the overlapping bins that ends after the linear index' offset of beg's 16 kb window.
template <class BinMap>
std::vector<Chunk> query_chunks(const BinMap& bins, const std::vector<uint64_t>& linear, int64_t beg, int64_t end) {
  std::vector<uint32_t> cand;
  reg2bins(beg, end, cand);
  uint64_t min_off = 0;
  if (!linear.empty()) min_off = linear[std::min<size_t>((size_t)(beg >> kLinearShift), linear.size() - 1)];
  std::vector<Chunk> todo;
  for (uint32_t bn : cand) {
    auto b = bins.find(bn);
    if (b == bins.end()) continue;
    for (const Chunk& c : b->second) if (c.end > min_off) todo.push_back(c);
  }
  std::sort(todo.begin(), todo.end(), [](const Chunk& a, const Chunk& b) { return a.beg < b.beg; });
  std::vector<Chunk> merged;
  for (const Chunk& c : todo) {
    if (!merged.empty() && c.beg <= merged.back().end) merged.back().end = std::max(merged.back().end, c.end);
    else merged.push_back(c);
  }
  return merged;
}

}  // namespace bgzf
}  // namespace ltr
