// restart_file.hpp -- the container of a checkpoint: one file per rank, 64-bit offsets throughout (the zip32 writer of state_io.hpp
// stays for gb25_save_state).  Layout, little-endian:
//   header (64 B)   magic "GB25RST\0", version, real_bytes, member count, scalar bytes, offsets of the scalar block, the table
//                   and the data, the size of the whole file
//   scalar block    the bytes of RestartScalars (restart_plan.hpp); the clock comes first: time, last_dt (f8), iteration (i8)
//   member table    one 128-byte row per member: name, field id, extra id, dims, element bytes, offset, bytes, arena offset, s1, s2
//   members         raw, each at a 64-byte-aligned offset
// Written to "<path>.tmp" and renamed when complete.  The reader believes no number of the table before it has checked it
// against the size of the file.  Also here: the host restatement of the two checksums.  Plain C++, no HIP (tests/test_restart_file.py).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fcntl.h>
#include <unistd.h>
#include <string>
#include <vector>

namespace {

constexpr char kRestartMagic[8] = {'G', 'B', '2', '5', 'R', 'S', 'T', 0};
constexpr uint32_t kRestartVersion = 1;
constexpr uint32_t kRestartMaxMembers = 4096, kRestartMaxScalarBytes = 1u << 20;

struct RestartFileHeader {
  char magic[8];
  uint32_t version, real_bytes, members, scalar_bytes;
  uint64_t scalars_offset, table_offset, data_offset, file_bytes;
  uint64_t reserved;
};
static_assert(sizeof(RestartFileHeader) == 64, "the header is 64 bytes");

struct RestartFileRow {
  char name[48];
  int32_t field, extra, dims[3], elem_bytes;
  uint64_t offset, bytes, arena_offset, s1, s2;
  uint64_t reserved[2];
};
static_assert(sizeof(RestartFileRow) == 128, "a row of the member table is 128 bytes");

// s1 = sum x_n, s2 = sum (n + 1) x_n, mod 2^64; x_n: the bit pattern of element n as an unsigned integer of its own width,
// n = elem0 + its index in p (elem0: where p starts in the member).  Adds to *s1, *s2.
inline void restart_checksums(const void* p, uint64_t count, int elem_bytes, uint64_t elem0, uint64_t* s1, uint64_t* s2) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  uint64_t a1 = 0, a2 = 0;
  for (uint64_t n = 0; n < count; n++) {
    uint64_t x = 0;
    if (elem_bytes == 8) memcpy(&x, b + 8 * n, 8);
    else { uint32_t y; memcpy(&y, b + 4 * n, 4); x = y; }
    a1 += x;
    a2 += (elem0 + n + 1) * x;
  }
  *s1 += a1;
  *s2 += a2;
}

inline uint64_t restart_align64(uint64_t b) { return (b + 63) & ~(uint64_t)63; }

// rows: name .. arena_offset, s1, s2 filled in by the caller; offset is assigned here.  The bytes of member q are read from
// arena + rows[q].arena_offset.
inline bool restart_write_file(const std::string& path, uint32_t real_bytes, const void* scalars, uint32_t scalar_bytes,
                               std::vector<RestartFileRow> rows, const unsigned char* arena, std::string* err) {
  RestartFileHeader h;
  memset(&h, 0, sizeof h);
  memcpy(h.magic, kRestartMagic, 8);
  h.version = kRestartVersion; h.real_bytes = real_bytes; h.members = (uint32_t)rows.size(); h.scalar_bytes = scalar_bytes;
  h.scalars_offset = sizeof h;
  h.table_offset = restart_align64(h.scalars_offset + scalar_bytes);
  h.data_offset = restart_align64(h.table_offset + rows.size() * sizeof(RestartFileRow));
  uint64_t at = h.data_offset;
  for (RestartFileRow& r : rows) { r.offset = at; at = restart_align64(at + r.bytes); }
  h.file_bytes = at;
  const std::string tmp = path + ".tmp";
  FILE* f = fopen(tmp.c_str(), "wb");
  if (!f) { *err = "cannot write " + tmp; return false; }
  static const unsigned char zeros[64] = {0};
  uint64_t pos = 0;
  auto put = [&](const void* p, uint64_t n) { pos += n; return n == 0 || fwrite(p, 1, n, f) == n; };
  auto pad_to = [&](uint64_t target) { return put(zeros, target - pos); };
  bool ok = put(&h, sizeof h) && put(scalars, scalar_bytes) && pad_to(h.table_offset) &&
            put(rows.data(), rows.size() * sizeof(RestartFileRow)) && pad_to(h.data_offset);
  for (size_t q = 0; ok && q < rows.size(); q++) ok = put(arena + rows[q].arena_offset, rows[q].bytes) && pad_to(restart_align64(pos));
  // (on stable storage before it takes the name of a checkpoint, and the directory entry after: a node that goes down must not
  // leave a renamed file without its data in the place of the last good one)
  ok = (fflush(f) == 0) && ok;
  ok = (fsync(fileno(f)) == 0) && ok;
  ok = (fclose(f) == 0) && ok;
  if (ok && rename(tmp.c_str(), path.c_str()) != 0) ok = false;
  if (ok) {
    const size_t slash = path.find_last_of('/');
    const int dir = ::open(slash == std::string::npos ? "." : path.substr(0, slash + 1).c_str(), O_RDONLY);
    if (dir >= 0) { (void)fsync(dir); ::close(dir); }
  }
  if (!ok) { remove(tmp.c_str()); *err = "writing " + path + " failed (disk full?)"; }
  return ok;
}

struct RestartFile {
  FILE* f = nullptr;
  RestartFileHeader header;
  std::vector<unsigned char> scalars;
  std::vector<RestartFileRow> rows;
  ~RestartFile() { if (f) fclose(f); }
  // header, scalar block and table, each checked against the size of the file before it is used
  bool open(const std::string& path, std::string* err) {
    const size_t n = path.size();
    if (n >= 4 && path.compare(n - 4, 4, ".tmp") == 0) { *err = path + ": an unfinished checkpoint (*.tmp) is no checkpoint"; return false; }
    f = fopen(path.c_str(), "rb");
    if (!f) { *err = "cannot read " + path; return false; }
    if (fseeko(f, 0, SEEK_END) != 0) { *err = path + ": cannot seek"; return false; }
    const uint64_t size = (uint64_t)ftello(f);
    rewind(f);
    if (size < sizeof header || fread(&header, 1, sizeof header, f) != sizeof header) { *err = path + ": shorter than a header"; return false; }
    if (memcmp(header.magic, kRestartMagic, 8) != 0) { *err = path + ": not a gb25 checkpoint (magic)"; return false; }
    if (header.version != kRestartVersion) { *err = path + ": format version " + std::to_string(header.version) + ", this library reads " + std::to_string(kRestartVersion); return false; }
    if (header.real_bytes != 4 && header.real_bytes != 8) { *err = path + ": real_bytes is neither 4 nor 8"; return false; }
    if (header.members == 0 || header.members > kRestartMaxMembers) { *err = path + ": member count " + std::to_string(header.members) + " out of bounds"; return false; }
    if (header.scalar_bytes > kRestartMaxScalarBytes) { *err = path + ": scalar block out of bounds"; return false; }
    if (header.file_bytes != size) { *err = path + ": truncated (" + std::to_string(size) + " bytes of " + std::to_string(header.file_bytes) + ")"; return false; }
    auto within = [size](uint64_t off, uint64_t len) { return off <= size && len <= size - off; };
    if (!within(header.scalars_offset, header.scalar_bytes)) { *err = path + ": the scalar block lies beyond the end of the file"; return false; }
    if (!within(header.table_offset, (uint64_t)header.members * sizeof(RestartFileRow))) { *err = path + ": the member table lies beyond the end of the file"; return false; }
    scalars.resize(header.scalar_bytes);
    if (fseeko(f, (off_t)header.scalars_offset, SEEK_SET) != 0 || fread(scalars.data(), 1, scalars.size(), f) != scalars.size()) { *err = path + ": cannot read the scalar block"; return false; }
    rows.resize(header.members);
    if (fseeko(f, (off_t)header.table_offset, SEEK_SET) != 0 || fread(rows.data(), 1, rows.size() * sizeof(RestartFileRow), f) != rows.size() * sizeof(RestartFileRow)) { *err = path + ": cannot read the member table"; return false; }
    for (RestartFileRow& r : rows) {
      r.name[sizeof r.name - 1] = 0;
      if (!within(r.offset, r.bytes) || r.offset < header.data_offset) { *err = path + ": member " + r.name + " lies beyond the end of the file"; return false; }
      if ((r.elem_bytes != 4 && r.elem_bytes != 8) || r.bytes % (uint64_t)r.elem_bytes != 0 || r.dims[0] < 0 || r.dims[1] < 0 || r.dims[2] < 0 ||
          (uint64_t)r.dims[0] * (uint64_t)r.dims[1] > (r.bytes / (uint64_t)r.elem_bytes) + 1 ||   // (no overflow in the product below)
          (uint64_t)r.dims[0] * (uint64_t)r.dims[1] * (uint64_t)r.dims[2] != r.bytes / (uint64_t)r.elem_bytes) {
        *err = path + ": member " + r.name + " states dims that are not its bytes"; return false;
      }
    }
    return true;
  }
  bool read_member(size_t q, uint64_t begin, uint64_t bytes, void* dst) {
    return begin <= rows[q].bytes && bytes <= rows[q].bytes - begin && fseeko(f, (off_t)(rows[q].offset + begin), SEEK_SET) == 0 &&
           fread(dst, 1, bytes, f) == bytes;
  }
};

}  // namespace
