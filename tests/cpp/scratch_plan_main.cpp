// The censuses' scratch carver and rows-per-wave plan (kaboodle_amd/csrc/kb_scratch.h) on their own: every carve
// aligned as asked, inside the total and apart from the others, the dry run's total equal to the real one's; the plan a
// multiple of its granule inside its bounds, its row tiles inside one grid dimension, and equal to the two formulas it
// replaced (restated here) wherever those kept the grid themselves.  Plain C++; tests/test_scratch_plan.py builds it
// with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../kaboodle_amd/csrc/kb_scratch.h"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct Piece { char* p; size_t off, bytes, align; };

// a layout of mixed types and alignments, the shape the censuses use: a cleared span in the middle
template <class T> static void piece(Carve& c, std::vector<Piece>& got, size_t n, size_t align) {
  T* p = c.take<T>(n, align);
  got.push_back(Piece{reinterpret_cast<char*>(p), c.bytes() - sizeof(T) * n, sizeof(T) * n, align});
}
static void lay(Carve& c, std::vector<Piece>& got, uint32_t seed) {
  uint32_t x = seed;
  auto rnd = [&](uint32_t m) { x = x * 1664525u + 1013904223u; return (x >> 8) % m; };
  piece<uint8_t>(c, got, 1 + rnd(300), 1);
  piece<uint32_t>(c, got, rnd(100), 16);
  c.zero_from();
  piece<unsigned long long>(c, got, 1 + rnd(40), 8);
  piece<uint32_t>(c, got, rnd(3) ? 3 * rnd(700) : 0, 4);
  piece<uint16_t>(c, got, 1 + rnd(999), 16);
  c.zero_to();
  piece<uint8_t>(c, got, rnd(77), 1);
  piece<uint32_t>(c, got, 1 + rnd(64), 256);
  piece<uint8_t>(c, got, 1 + rnd(5), 1);
}

// the two formulas before they became one: the view census's (it had no grid guard) and the delta census's
static uint32_t old_cs_rpw(uint64_t R, uint32_t cb, uint32_t ncu, uint64_t want) {
  uint64_t rpw = (R * cb + 16ull * ncu - 1) / (16ull * ncu);
  if (want) rpw = want;
  rpw = std::min<uint64_t>(std::max<uint64_t>((rpw + 24 - 1) / 24 * 24, 24), 4080);
  return (uint32_t)rpw;
}
static uint32_t old_dl_rpw(uint64_t R, uint32_t cb, uint32_t ncu, uint64_t want) {
  uint64_t rpw = want ? want : (R * cb + 16ull * ncu - 1) / (16ull * ncu);
  rpw = std::min<uint64_t>(std::max<uint64_t>((rpw + 8 - 1) / 8 * 8, 8), 4080);
  while (rpw < 4080 && (R + 4 * rpw - 1) / (4 * rpw) > 65535) rpw = std::min<uint64_t>(rpw * 2, 4080);
  return (uint32_t)rpw;
}
// unmoved: the view census's plan is the old one (its guard did not act)
static bool plan_ok(uint64_t R, uint32_t cb, uint32_t ncu, uint64_t want, bool unmoved = false) {
  const uint32_t cs = rows_per_wave(R, cb, ncu, want, 24, 4080), dl = rows_per_wave(R, cb, ncu, want, 8, 4080);
  if (cs % 24 || cs < 24 || cs > 4080 || dl % 8 || dl < 8 || dl > 4080) return false;
  if (row_tiles(R, cs) > GRID_DIM_MAX || row_tiles(R, dl) > GRID_DIM_MAX || row_tiles(R, cs) * 4ull * cs < R) return false;
  if (dl != old_dl_rpw(R, cb, ncu, want)) return false;
  const uint32_t oc = old_cs_rpw(R, cb, ncu, want);
  const bool guarded = (R + 4ull * oc - 1) / (4ull * oc) > GRID_DIM_MAX;   // the old plan would have overrun the grid
  return guarded ? !unmoved && cs > oc : cs == oc;
}

int main() {
  for (uint32_t seed = 0; seed < 200; ++seed) {
    std::vector<Piece> dry, real;
    Carve d;
    lay(d, dry, seed);
    CHECK(d.bytes() > 0 && d.zero_bytes() <= d.bytes());
    for (const Piece& q : dry) CHECK(q.p == nullptr);
    // the base as aligned as the largest alignment asked for; ASan's redzones start right after the total
    char* buf = static_cast<char*>(aligned_alloc(256, (d.bytes() + 255) / 256 * 256));
    CHECK(buf);
    Carve c(buf);
    lay(c, real, seed);
    CHECK(c.bytes() == d.bytes() && c.z0 == d.z0 && c.z1 == d.z1 && real.size() == dry.size());
    CHECK(c.z0 % 16 == 0 && static_cast<char*>(c.zero_ptr()) == buf + c.z0);
    size_t end = 0;
    for (size_t k = 0; k < real.size(); ++k) {
      const Piece& q = real[k];
      CHECK(q.off == dry[k].off && q.bytes == dry[k].bytes && q.p == buf + q.off);
      CHECK(reinterpret_cast<uintptr_t>(q.p) % q.align == 0);
      CHECK(q.off >= end && q.off + q.bytes <= c.bytes());            // in order, apart, inside the total
      end = q.off + q.bytes;
      memset(q.p, 0xA5, q.bytes);
    }
    memset(c.zero_ptr(), 0, c.zero_bytes());                          // clears pieces 2..4 whole and nothing else
    for (size_t k = 0; k < real.size(); ++k)
      for (size_t b = 0; b < real[k].bytes; ++b) CHECK((unsigned char)real[k].p[b] == (k >= 2 && k <= 4 ? 0x00 : 0xA5));
    free(buf);
  }
  CHECK(carve_bytes([](Carve& c) { c.take<uint32_t>(3); c.take<uint64_t>(1, 16); }) == 24);

  // the default plan over every row count: the view census's never needs the guard (cb >= 1, 16-bit grid, ncu CUs)
  const uint32_t cbs[] = {1, 3, 2048};
  for (uint32_t cb : cbs)
    for (uint64_t R = 1; R <= (1ull << 24); ++R) {
      if (!plan_ok(R, cb, 256, 0, true)) { std::printf("FAILED plan R=%llu cb=%u\n", (unsigned long long)R, cb); return 1; }
    }
  // other CU counts and the override (a knob can ask for few rows a wave: there the guard acts), on a coarser sweep
  const uint32_t ncus[] = {1, 64, 304};
  const uint64_t wants[] = {1, 8, 24, 25, 512, 4080, 5000, 1ull << 40};
  for (uint32_t ncu : ncus)
    for (uint32_t cb : cbs)
      for (uint64_t R = 1; R <= (1ull << 24); R += 1 + R / 64) {
        CHECK(plan_ok(R, cb, ncu, 0, true));
        for (uint64_t w : wants) CHECK(plan_ok(R, cb, ncu, w));
      }
  CHECK(rows_per_wave(1ull << 24, 1, 256, 1, 24, 4080) == 96);        // 24 rows a wave would be 174,763 tiles
  CHECK(row_tiles(1ull << 24, 96) == 43691 && row_tiles(0, 8) == 0 && row_tiles(1, 8) == 1 && row_tiles(33, 8) == 2);
  std::printf("scratch plan ok\n");
  return 0;
}
