// kb_scratch.h — how a census lays out its scratch and sizes its row tiles (DESIGN.md "Host control plane").  Plain
// C++ with no HIP in it (tests/cpp/scratch_plan_main.cpp builds it stand-alone); kb_bitpass.h includes it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

// A bump carver over one allocation.  take<T>(n, align): the next n elements of T at a multiple of `align` bytes from
// the base, which is itself aligned to the largest alignment asked for (device allocations: 256).  Without a base it
// is a dry run: every pointer is null and only bytes() counts.  zero_from() .. zero_to() bracket what a pass clears.
struct Carve {
  char* base;
  size_t at = 0, z0 = 0, z1 = 0;
  explicit Carve(void* b = nullptr) : base(static_cast<char*>(b)) {}
  template <class T> T* take(size_t n, size_t align = alignof(T)) {
    at = (at + align - 1) / align * align;
    T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;
    at += sizeof(T) * n;
    return p;
  }
  void zero_from(size_t align = 16) { at = (at + align - 1) / align * align; z0 = z1 = at; }
  void zero_to() { z1 = at; }
  void* zero_ptr() const { return base + z0; }    // not on a dry run
  size_t zero_bytes() const { return z1 - z0; }
  size_t bytes() const { return at; }
};
// `lay(Carve&)` over the allocation at `buf`; without one, the bytes the layout takes
template <class F> static Carve carve(void* buf, F&& lay) { Carve c(buf); lay(c); return c; }
template <class F> static size_t carve_bytes(F&& lay) { return carve(nullptr, lay).bytes(); }

// Rows per wave of a streaming pass (grid: column blocks x row tiles of 4 waves): about 16 waves a CU unless want != 0;
// a multiple of `granule` in [granule, max] (a multiple too), doubled while the tiles overrun one grid dimension.
constexpr uint32_t GRID_DIM_MAX = 65535;
static uint32_t rows_per_wave(uint64_t rows, uint32_t col_blocks, uint32_t ncu, uint64_t want, uint32_t granule, uint32_t max) {
  uint64_t rpw = want ? want : (rows * col_blocks + 16ull * ncu - 1) / (16ull * ncu);
  rpw = std::min<uint64_t>(std::max<uint64_t>((rpw + granule - 1) / granule * granule, granule), max);
  while (rpw < max && (rows + 4 * rpw - 1) / (4 * rpw) > GRID_DIM_MAX) rpw = std::min<uint64_t>(rpw * 2, max);
  return (uint32_t)rpw;
}
static uint32_t row_tiles(uint64_t rows, uint32_t rpw) { return (uint32_t)((rows + 4ull * rpw - 1) / (4ull * rpw)); }
// an environment knob that overrides the rows per wave (for measurements: results do not depend on it); 0 = not set
static uint64_t rpw_env(const char* name) { const char* ev = getenv(name); return ev ? (uint64_t)std::max<long long>(atoll(ev), 1) : 0; }
