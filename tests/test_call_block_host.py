"""gmr_amd/csrc/call_block.h without a GPU: a stand-alone C++ program (its own main, built with the host compiler under
AddressSanitizer and UBSan, never loaded into Python) reserves uploaded and device-only arrays of several element types in mixed
order and checks the layout the member-wise calls and the model image rely on."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gmr_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "call_block.h"

using gmr::CallBlock;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

struct Big { double d[26]; int tag; };  // 216 bytes, like one member's entry
static_assert(sizeof(Big) > 200 && sizeof(Big) % 16 != 0, "an entry-sized struct that is no multiple of 16 bytes");

struct Span { size_t at, bytes; bool device_only; };  // where an array came to lie, from its resolved pointer

struct Book {
  CallBlock blk;
  std::vector<Span> spans;  // filled by note()
  template <class T> CallBlock::Uploaded<T> up(size_t n) {
    auto h = blk.uploaded<T>(n);
    CHECK(h.n == n);
    return h;
  }
};

template <class H>
static void note(Book &b, const CallBlock::Device &dev, uint8_t *base, H h, size_t elem, bool device_only) {
  uint8_t *p = reinterpret_cast<uint8_t *>(dev(h));
  CHECK(p >= base);
  b.spans.push_back({(size_t)(p - base), h.n * elem, device_only});
}

static void check_layout(const Book &b) {
  const size_t up = b.blk.uploaded_bytes(), total = b.blk.total_bytes();
  CHECK(up <= total);
  for (size_t i = 0; i < b.spans.size(); ++i) {
    const Span &s = b.spans[i];
    CHECK(s.at % 16 == 0);
    CHECK(s.at + s.bytes <= total);
    if (s.device_only) CHECK(s.at >= up);
    else CHECK(s.at + s.bytes <= up);
    for (size_t j = 0; j < i; ++j) {
      const Span &t = b.spans[j];
      CHECK(s.at + s.bytes <= t.at || t.at + t.bytes <= s.at || s.bytes == 0 || t.bytes == 0);
    }
  }
}

// uploaded and device-only arrays of 0, 1 and several elements of the four types, interleaved
static void mixed(int variant) {
  Book b;
  const size_t counts[] = {0, 1, 3, 7, 2, 0, 5, 1};
  std::vector<CallBlock::Uploaded<int>> ui;
  std::vector<CallBlock::Uploaded<int64_t>> ul;
  std::vector<CallBlock::Uploaded<double>> ud;
  std::vector<CallBlock::Uploaded<Big>> ub;
  std::vector<CallBlock::DeviceOnly<int>> di;
  std::vector<CallBlock::DeviceOnly<int64_t>> dl;
  std::vector<CallBlock::DeviceOnly<double>> dd;
  std::vector<CallBlock::DeviceOnly<Big>> db;
  for (int k = 0; k < 24; ++k) {
    const size_t n = counts[(k + variant) % 8];
    const int type = (k * 5 + variant) % 4;
    const bool device_only = ((k + variant) % 3) == 1;
    if (device_only) {
      if (type == 0) di.push_back(b.blk.device_only<int>(n));
      if (type == 1) dl.push_back(b.blk.device_only<int64_t>(n));
      if (type == 2) dd.push_back(b.blk.device_only<double>(n));
      if (type == 3) db.push_back(b.blk.device_only<Big>(n));
    } else {
      if (type == 0) ui.push_back(b.up<int>(n));
      if (type == 1) ul.push_back(b.up<int64_t>(n));
      if (type == 2) ud.push_back(b.up<double>(n));
      if (type == 3) ub.push_back(b.up<Big>(n));
    }
  }
  CHECK(!ui.empty() && !ul.empty() && !ud.empty() && !ub.empty() && !di.empty() && !dl.empty() && !dd.empty() && !db.empty());
  // write every second int array and the first struct array; everything else must stay zero
  std::vector<uint8_t> expect(b.blk.uploaded_bytes(), 0);
  for (size_t a = 0; a < ui.size(); a += 2)
    for (size_t i = 0; i < ui[a].n; ++i) {
      b.blk[ui[a]][i] = 0x01010101 * (int)(a + 1);
      memset(expect.data() + ui[a].at + 4 * i, (int)(a + 1), 4);
    }
  for (size_t i = 0; i < ub[0].n; ++i) {
    memset(&b.blk[ub[0]][i], 0x5a, sizeof(Big));
    memset(expect.data() + ub[0].at + sizeof(Big) * i, 0x5a, sizeof(Big));
  }
  CHECK(memcmp(b.blk.image(), expect.data(), expect.size()) == 0);

  alignas(16) static uint8_t arena[1 << 16];  // stands for the device allocation: only addresses are taken
  CHECK(b.blk.total_bytes() <= sizeof(arena));
  uint8_t *base = arena + 16 * variant;
  const CallBlock::Device dev = b.blk.on(base);
  for (auto h : ui) { note(b, dev, base, h, sizeof(int), false); CHECK(reinterpret_cast<uint8_t *>(dev(h)) == base + h.at); }
  for (auto h : ul) { note(b, dev, base, h, sizeof(int64_t), false); CHECK(reinterpret_cast<uint8_t *>(dev(h)) == base + h.at); }
  for (auto h : ud) { note(b, dev, base, h, sizeof(double), false); CHECK(reinterpret_cast<uint8_t *>(dev(h)) == base + h.at); }
  for (auto h : ub) { note(b, dev, base, h, sizeof(Big), false); CHECK(reinterpret_cast<uint8_t *>(dev(h)) == base + h.at); }
  const size_t tail = (b.blk.uploaded_bytes() + 15) / 16 * 16;
  for (auto h : di) { note(b, dev, base, h, sizeof(int), true); CHECK(reinterpret_cast<uint8_t *>(dev(h)) == base + tail + h.at); }
  for (auto h : dl) { note(b, dev, base, h, sizeof(int64_t), true); CHECK(reinterpret_cast<uint8_t *>(dev(h)) == base + tail + h.at); }
  for (auto h : dd) { note(b, dev, base, h, sizeof(double), true); CHECK(reinterpret_cast<uint8_t *>(dev(h)) == base + tail + h.at); }
  for (auto h : db) { note(b, dev, base, h, sizeof(Big), true); CHECK(reinterpret_cast<uint8_t *>(dev(h)) == base + tail + h.at); }
  CHECK(b.spans.size() == 24);
  check_layout(b);
  // the host image of an uploaded array is the block's image at the array's device offset
  for (auto h : ul) CHECK(reinterpret_cast<const uint8_t *>(b.blk[h]) == static_cast<const uint8_t *>(b.blk.image()) + h.at);
}

static void edges() {
  alignas(16) static uint8_t arena[4096];
  {  // an empty block
    CallBlock blk;
    CHECK(blk.uploaded_bytes() == 0 && blk.total_bytes() == 0);
    (void)blk.on(arena);
  }
  {  // empty arrays only
    Book b;
    auto u = b.up<double>(0);
    auto d = b.blk.device_only<Big>(0);
    CHECK(b.blk.uploaded_bytes() == 0 && b.blk.total_bytes() == 0);
    const CallBlock::Device dev = b.blk.on(arena);
    note(b, dev, arena, u, sizeof(double), false);
    note(b, dev, arena, d, sizeof(Big), true);
    check_layout(b);
  }
  {  // device-only arrays only: nothing to upload
    Book b;
    auto k = b.blk.device_only<int>(5);
    auto r = b.blk.device_only<int64_t>(3);
    auto g = b.blk.device_only<Big>(1);
    CHECK(b.blk.uploaded_bytes() == 0);
    CHECK(b.blk.total_bytes() == 64 + sizeof(Big));
    const CallBlock::Device dev = b.blk.on(arena);
    note(b, dev, arena, k, sizeof(int), true);
    note(b, dev, arena, r, sizeof(int64_t), true);
    note(b, dev, arena, g, sizeof(Big), true);
    CHECK(reinterpret_cast<uint8_t *>(dev(k)) == arena && reinterpret_cast<uint8_t *>(dev(r)) == arena + 32);
    check_layout(b);
  }
  {  // a device-only array reserved first still lies behind an uploaded one reserved after it
    Book b;
    auto d = b.blk.device_only<int>(3);
    auto u = b.up<Big>(2);
    CHECK(b.blk.uploaded_bytes() == 2 * sizeof(Big));
    CHECK(b.blk.total_bytes() == (2 * sizeof(Big) + 15) / 16 * 16 + 12);
    const CallBlock::Device dev = b.blk.on(arena);
    note(b, dev, arena, d, sizeof(int), true);
    note(b, dev, arena, u, sizeof(Big), false);
    CHECK(reinterpret_cast<uint8_t *>(dev(u)) == arena);
    check_layout(b);
  }
  {  // put: a copy of a vector, padded with zeros to min_n elements
    CallBlock blk;
    auto a = blk.put(std::vector<int64_t>{7, -1, 1ll << 40});
    auto e = blk.put(std::vector<double>{}, 1);
    auto s = blk.put(std::vector<int>{3}, 4);
    CHECK(a.n == 3 && e.n == 1 && s.n == 4);
    CHECK(blk[a][0] == 7 && blk[a][1] == -1 && blk[a][2] == (1ll << 40));
    CHECK(blk[e][0] == 0.0);
    CHECK(blk[s][0] == 3 && blk[s][1] == 0 && blk[s][3] == 0);
    CHECK(a.at == 0 && e.at == 32 && s.at == 48 && blk.uploaded_bytes() == 64 && blk.total_bytes() == 64);
  }
}

int main() {
  for (int v = 0; v < 12; ++v) mixed(v);
  edges();
  puts("ok");
  return 0;
}
"""


def test_call_block_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src, exe = tmp_path / "call_block_test.cpp", tmp_path / "call_block_test"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{CSRC}", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_call_block_header_is_host_only():
    """Plain C++ with no HIP include, as the stand-alone build above needs."""
    text = open(os.path.join(CSRC, "call_block.h")).read()
    assert "hip" not in "\n".join(ln for ln in text.split("\n") if ln.lstrip().startswith("#include"))
