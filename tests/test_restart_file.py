"""The checkpoint container (csrc/restart_file.hpp) and its numpy reader (gb25_amd/restart.py): a small stand-alone program with its
own main writes a file, reads files back and restates the checksums; the Python reader reads the same files.  The program is built
once more with -fsanitize=address,undefined and run over the same good and malformed files (a plain executable on the CPU).
No GPU, no library."""
import os
import struct
import subprocess

import numpy as np
import pytest

from gb25_amd import restart

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include "gb-25_amd/csrc/restart_file.hpp"
#include <cstdlib>
// write <path>: three members (f4 of 5 x 3 x 2, f8 of 7 x 1 x 1, f4 of 1 x 1 x 1), values k * 0.5 - 3, scalars "time, last_dt, iteration"
// read <path>: print the scalars, every row and its checksums as read, or "refused <why>"
// sums <file of raw bytes> <elem_bytes>: the checksums of the bytes
int main(int argc, char** argv) {
  const std::string mode = argv[1], path = argv[2];
  std::string err;
  if (mode == "write") {
    const int dims[3][3] = {{5, 3, 2}, {7, 1, 1}, {1, 1, 1}}, eb[3] = {4, 8, 4};
    std::vector<unsigned char> arena;
    std::vector<RestartFileRow> rows(3);
    for (int q = 0; q < 3; q++) {
      RestartFileRow& r = rows[q];
      memset(&r, 0, sizeof r);
      snprintf(r.name, sizeof r.name, "member%d", q);
      r.field = q; r.extra = -1; r.elem_bytes = eb[q];
      uint64_t n = 1;
      for (int a = 0; a < 3; a++) { r.dims[a] = dims[q][a]; n *= dims[q][a]; }
      r.bytes = n * eb[q];
      r.arena_offset = (arena.size() + 15) / 16 * 16;
      arena.resize(r.arena_offset + r.bytes);
      for (uint64_t k = 0; k < n; k++) {
        if (eb[q] == 4) { float x = k * 0.5f - 3; memcpy(&arena[r.arena_offset + 4 * k], &x, 4); }
        else { double x = k * 0.5 - 3; memcpy(&arena[r.arena_offset + 8 * k], &x, 8); }
      }
      restart_checksums(&arena[r.arena_offset], n, eb[q], 0, &r.s1, &r.s2);
    }
    struct { double time, last_dt; int64_t iteration; char more[40]; } scalars = {86400.5, 600.0, 144, "the rest of the scalar block"};
    if (!restart_write_file(path, 4, &scalars, sizeof scalars, rows, arena.data(), &err)) { printf("failed %s\n", err.c_str()); return 1; }
    return 0;
  }
  if (mode == "read") {
    RestartFile f;
    if (!f.open(path, &err)) { printf("refused %s\n", err.c_str()); return 0; }
    double t[2]; int64_t it;
    memcpy(t, f.scalars.data(), 16); memcpy(&it, f.scalars.data() + 16, 8);
    printf("scalars %.17g %.17g %lld %u\n", t[0], t[1], (long long)it, f.header.real_bytes);
    for (size_t q = 0; q < f.rows.size(); q++) {
      const RestartFileRow& r = f.rows[q];
      std::vector<unsigned char> b(r.bytes);
      if (!f.read_member(q, 0, r.bytes, b.data())) { printf("refused member %s unreadable\n", r.name); return 0; }
      uint64_t s1 = 0, s2 = 0;
      // (in two runs, the second from where the first ended: what a piece of a bounded arena does)
      const uint64_t n = r.bytes / r.elem_bytes, half = n / 2;
      restart_checksums(b.data(), half, r.elem_bytes, 0, &s1, &s2);
      restart_checksums(b.data() + half * r.elem_bytes, n - half, r.elem_bytes, half, &s1, &s2);
      printf("row %s %d %d %d %d %d %d %llu %llu %llu %llu %llu %llu\n", r.name, r.field, r.extra, r.dims[0], r.dims[1], r.dims[2], r.elem_bytes,
             (unsigned long long)r.offset, (unsigned long long)r.bytes, (unsigned long long)r.s1, (unsigned long long)r.s2,
             (unsigned long long)s1, (unsigned long long)s2);
    }
    return 0;
  }
  if (mode == "sums") {
    const int eb = atoi(argv[3]);
    FILE* f = fopen(path.c_str(), "rb");
    std::vector<unsigned char> b;
    unsigned char buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) b.insert(b.end(), buf, buf + n);
    fclose(f);
    uint64_t s1 = 0, s2 = 0;
    restart_checksums(b.data(), b.size() / eb, eb, 0, &s1, &s2);
    printf("%llu %llu\n", (unsigned long long)s1, (unsigned long long)s2);
    return 0;
  }
  return 2;
}
"""


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("restart_file_" + request.param)
    src = d / "main.cpp"
    src.write_text(MAIN)
    exe = d / "restart_file"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else ["-O1"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unused-const-variable", "-I", ROOT, str(src), "-o", str(exe)] + flags, check=True)

    def run(*args):
        r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr   # (a sanitizer report ends the program with a failure)
        return r.stdout.splitlines()
    run.dir = d
    return run


@pytest.fixture
def good(program):
    path = program.dir / "restart_rank0.gb25"
    program("write", path)
    return path


def expected_member(q):
    dims, dtype = [((5, 3, 2), np.float32), ((7, 1, 1), np.float64), ((1, 1, 1), np.float32)][q]
    n = int(np.prod(dims))
    return (np.arange(n, dtype=dtype) * dtype(0.5) - dtype(3)).reshape(dims, order="F")


def test_round_trip(program, good):
    assert not os.path.exists(str(good) + ".tmp")
    lines = program("read", good)
    assert lines[0].split() == ["scalars", "86400.5", "600", "144", "4"]
    c = restart.read_checkpoint(good)
    assert (c.time, c.last_dt, c.iteration, c.real_bytes) == (86400.5, 600.0, 144, 4) and c.names() == ["member0", "member1", "member2"]
    for q, ln in enumerate(lines[1:]):
        w = ln.split()
        want = expected_member(q)
        assert w[1] == f"member{q}" and [int(x) for x in w[2:8]] == [q, -1, *want.shape, want.dtype.itemsize]
        assert int(w[8]) % 64 == 0 and int(w[9]) == want.nbytes
        assert w[10:12] == w[12:14], "the sums recorded are the sums of the bytes read (taken in two runs)"
        got = c[f"member{q}"]
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(np.asarray(got), want)
        assert restart.checksums(got) == (int(w[10]), int(w[11])) == (c.table[f"member{q}"]["s1"], c.table[f"member{q}"]["s2"])
    assert restart.verify(good) == []


ARRAYS = {
    "length_1": np.array([2.5], dtype=np.float32),
    "length_3": np.array([1.0, -2.0, 3.0], dtype=np.float32),
    "length_7_f4": np.linspace(-1, 1, 7).astype(np.float32),
    "length_5_f8": np.linspace(-1, 1, 5),
    "special_f4": np.array([0x7FC00000, 0xFFC00001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000], dtype=np.uint32).view(np.float32),
    "special_f8": np.array([0x7FF8000000000000, 0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF], dtype=np.uint64).view(np.float64),
    # s2 wraps 2^64: 70000 elements near 2^63 each, weights up to 70000
    "wraps_f8": (np.arange(70000, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) | np.uint64(1 << 63)).view(np.float64),
    "wraps_f4": (np.arange(300000, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 32)).astype(np.uint32).view(np.float32),
}


@pytest.mark.parametrize("name", sorted(ARRAYS))
def test_checksums_equal_the_host_restatement(program, name):
    a = ARRAYS[name]
    raw = program.dir / (name + ".raw")
    raw.write_bytes(a.tobytes())
    s1, s2 = (int(x) for x in program("sums", raw, a.dtype.itemsize)[0].split())
    assert restart.checksums(a) == (s1, s2)
    x = [int(v) for v in a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)]
    if len(x) <= 10 or name == "wraps_f8":   # the definition, in Python integers
        assert s1 == sum(x) % 2**64 and s2 == sum((n + 1) * v for n, v in enumerate(x)) % 2**64
    if name == "wraps_f8":
        assert sum((n + 1) * v for n, v in enumerate(x)) >= 2**64


def damaged(good, name, edit):
    raw = bytearray(open(good, "rb").read())
    raw = edit(raw)
    path = os.path.join(os.path.dirname(str(good)), name + ".gb25")
    open(path, "wb").write(bytes(raw))
    return path


# header: magic 8 | version, real_bytes, members, scalar_bytes (4 x u32) | scalars, table, data offsets, file bytes (4 x u64)
MALFORMED = {
    "truncated": (lambda r: r[:len(r) - 100], "truncated"),
    "shorter_than_a_header": (lambda r: r[:40], "shorter than a header"),
    "wrong_magic": (lambda r: b"GB25RSX\0" + r[8:], "magic"),
    "wrong_version": (lambda r: r[:8] + struct.pack("<I", 9) + r[12:], "version"),
    "table_beyond_the_end": (lambda r: r[:32] + struct.pack("<Q", len(r) - 64) + r[40:], "member table lies beyond"),
    "member_beyond_the_end": (lambda r: r[:struct.unpack_from("<Q", r, 32)[0] + 72] + struct.pack("<Q", len(r) - 8)
                              + r[struct.unpack_from("<Q", r, 32)[0] + 80:], "member0 lies beyond"),
    "two_to_the_31_members": (lambda r: r[:16] + struct.pack("<I", 2**31) + r[20:], "member count 2147483648 out of bounds"),
    "dims_that_are_not_the_bytes": (lambda r: r[:struct.unpack_from("<Q", r, 32)[0] + 56] + struct.pack("<i", 6)
                                    + r[struct.unpack_from("<Q", r, 32)[0] + 60:], "dims that are not its bytes"),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_files_are_refused(program, good, case):
    edit, why = MALFORMED[case]
    path = damaged(good, case, edit)
    out = program("read", path)
    assert out[0].startswith("refused ") and why in out[0], out
    with pytest.raises(restart.CheckpointError, match=why):
        restart.read_checkpoint(path)


def test_an_unfinished_file_is_no_checkpoint(program, good):
    tmp = str(good) + ".tmp"
    open(tmp, "wb").write(open(good, "rb").read())
    assert "unfinished" in program("read", tmp)[0]
    with pytest.raises(restart.CheckpointError, match="unfinished"):
        restart.read_checkpoint(tmp)
    os.remove(tmp)


def test_a_flipped_byte_is_found(program, good):
    c = restart.read_checkpoint(good)
    path = damaged(good, "flipped", lambda r: r[:c.table["member1"]["offset"] + 3] + bytes([r[c.table["member1"]["offset"] + 3] ^ 4])
                   + r[c.table["member1"]["offset"] + 4:])
    assert restart.verify(path) == ["member1"]
    w = program("read", path)[2].split()
    assert w[10:12] != w[12:14]
