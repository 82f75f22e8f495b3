"""CPU: the scratch layout helper (map-oxidize_amd/csrc/mox_carve.h).  A small
C++ program of its own, built with the address and undefined-behaviour
sanitizers and run as a child process: pseudo-random layouts, and the tail of
the bytewise sort's scratch for an odd number of words (a 4 n-byte array in
front of 8-byte atomics)."""
import os
import subprocess

from srcpins import ROOT

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mox_carve.h"

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint64_t next() {  // xorshift64*
  rng ^= rng >> 12;
  rng ^= rng << 25;
  rng ^= rng >> 27;
  return rng * 0x2545F4914F6CDD1Dull;
}
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "line %d: %s (layout %d)\n", __LINE__, #cond, it); \
      return 1;                                                          \
    }                                                                    \
  } while (0)

struct Arr {
  size_t count, elem, align;
  uint8_t* p;
};

static uint8_t* take(Carve& c, const Arr& a) {
  switch (a.elem) {
    case 1: return c.take_bytes(a.count, a.align);
    case 4: return (uint8_t*)c.take<uint32_t>(a.count, a.align);
    case 8: return (uint8_t*)c.take<uint64_t>(a.count, a.align);
    default: return (uint8_t*)c.take<__int128>(a.count, a.align);
  }
}

// the tail of bsort_once's scratch (mox_bsort.hip) behind the six big arrays
struct Tail {
  uint8_t *pos, *lrun, *tick, *gh, *gs, *ssum, *total, *err;
};
static void tail(Carve& c, uint64_t n, Tail& t) {
  const uint64_t ntiles = (n + 4095) / 4096;
  t.pos = (uint8_t*)c.take<uint32_t>(n);  // the last big array: 4 n bytes
  t.lrun = (uint8_t*)c.take<uint64_t>(n / 4 + 16);
  t.tick = c.take_bytes(64 + 8 * 8 * 256 * ntiles);  // the tickets and, 64 bytes on, the status words
  t.gh = (uint8_t*)c.take<unsigned long long>(8 * 256);
  t.gs = (uint8_t*)c.take<uint64_t>(8 * 256);
  t.ssum = c.take_bytes(8 * (n / 2048 + 9));
  t.total = (uint8_t*)c.take<uint64_t>(8);
  t.err = (uint8_t*)c.take<unsigned int>(48);
}

int main() {
  static const size_t ELEMS[] = {1, 4, 8, 16}, ALIGNS[] = {8, 16, 256};
  int it = 0;
  for (; it < 400; it++) {
    std::vector<Arr> arrs(1 + next() % 9);
    for (Arr& a : arrs) {
      a.count = next() % 5 == 0 ? 0 : next() % 5001;
      a.elem = ELEMS[next() % 4];
      a.align = ALIGNS[next() % 3];
    }
    Carve size;
    for (Arr& a : arrs) {
      const size_t before = size.used;
      take(size, a);
      CHECK(a.count || size.used == before);  // a zero-length take consumes nothing
      CHECK(size.used >= before + a.count * a.elem);
    }
    // a buffer of exactly `used` bytes, 256-byte aligned as the device's are: the sanitizer sees any byte outside it
    void* raw = nullptr;
    CHECK(posix_memalign(&raw, 256, size.used ? size.used : 1) == 0);
    uint8_t* base = (uint8_t*)raw;
    Carve place{base};
    for (Arr& a : arrs) {
      const size_t before = place.used;
      a.p = take(place, a);
      CHECK(a.count || place.used == before);
      CHECK((uintptr_t)a.p % a.align == 0);
      CHECK((uintptr_t)a.p % a.elem == 0 || a.elem > a.align);
      CHECK(a.p >= base + before && a.p < base + before + a.align);  // the next aligned position behind what was taken
      CHECK(!a.count || a.p + a.count * a.elem == base + place.used);  // inside the buffer (an empty array lies nowhere)
      if (a.count) memset(a.p, 0x5A, a.count * a.elem);
    }
    CHECK(place.used == size.used);  // the sizing pass and the placing pass agree
    for (size_t i = 0; i < arrs.size(); i++)
      for (size_t j = i + 1; j < arrs.size(); j++) {
        const Arr &a = arrs[i], &b = arrs[j];
        if (a.count && b.count) CHECK(a.p + a.count * a.elem <= b.p);  // disjoint, in the order taken
      }
    free(raw);
  }
  // an odd number of words: every array behind the 4 n-byte one stays aligned for its 8-byte atomics
  for (uint64_t n : {3ull, 4097ull, 1025ull, 99999ull, 1ull, 5ull}) {
    Tail s{}, t{};
    Carve size;
    tail(size, n, s);
    void* raw = nullptr;
    CHECK(posix_memalign(&raw, 256, size.used) == 0);
    Carve place{(uint8_t*)raw};
    tail(place, n, t);
    CHECK(place.used == size.used);
    for (uint8_t* p : {t.lrun, t.tick, t.tick + 64, t.gh, t.gs, t.ssum, t.total}) CHECK((uintptr_t)p % 8 == 0);
    CHECK((uintptr_t)t.err % 4 == 0 && (uintptr_t)t.pos % 4 == 0);
    CHECK(t.lrun >= t.pos + 4 * n && t.err + 192 == place.base + place.used);
    memset(place.base, 0, place.used);
    free(raw);
  }
  printf("carve ok: %d layouts\n", it);
  return 0;
}
"""


def test_carve_layouts_under_the_sanitizers(tmp_path):
    src, exe = tmp_path / "carve_check.cpp", tmp_path / "carve_check"
    src.write_text(PROGRAM)
    inc = os.path.join(ROOT, "map-oxidize_amd", "csrc")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", inc, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.strip() == "carve ok: 400 layouts"
