// Slot arithmetic of k_s1's re-scoring ring (km_screen1.hip, tail()).
//
// A wave keeps `rc` rows (rc < ring) in its ring between tiles.  A tile adds
// nn <= S1_TILE_ROWS rows, ranked rk = 0 .. nn - 1 in row order.  The rows
// are numbered on from the ring's fill, p = rc + rk: batch p / ring is
// re-scored as soon as it is full (p / ring = 0: the batch that holds the
// rows carried in), and row p sits in slot p % ring of it.  After the tile the
// ring holds (rc + nn) % ring rows, the last, partial batch.  With
// ring >= S1_TILE_ROWS a tile fills at most one batch; a 12-slot ring (the
// twelve-wave geometries) can be filled twice by one tile (rc = 8, nn = 16),
// so the kernel re-scores up to S1_RING_MAX_FULL batches per tile.
//
// Plain C++ (no HIP headers): the exhaustive check below is compiled into
// every build of the library, host and device pass alike.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KM_S1_RING_FN __host__ __device__ constexpr
#else
#define KM_S1_RING_FN constexpr
#endif

namespace km {

constexpr uint32_t S1_TILE_ROWS = 16;     // rows of a tile = the most a tile can add
constexpr uint32_t S1_RING_MAX_FULL = 2;  // full batches one tile can complete

struct S1RingSlot {
  uint32_t batch;  // 0: stashed before the first re-score of the tile, b: after the b-th
  uint32_t slot;   // < ring
  uint32_t rc;     // rows left in the ring after the tile (< ring)
};

// p = batch * ring + slot for p < 3 ring, by comparison (no division in the kernel)
KM_S1_RING_FN uint32_t s1_ring_batch(uint32_t ring, uint32_t p) {
  return (p >= ring ? 1u : 0u) + (p >= 2u * ring ? 1u : 0u);
}

// the place of the needy row of rank rk (rk < nn; rk = nn: the first free
// place after the tile, whose batch is the number of full batches) of a tile
// with nn needy rows, for a ring holding rc rows.  Needs rc < ring and
// nn <= S1_TILE_ROWS <= 2 ring, so that rc + nn < 3 ring.
KM_S1_RING_FN S1RingSlot s1_ring_slot(uint32_t ring, uint32_t rc, uint32_t nn, uint32_t rk) {
  const uint32_t p = rc + rk, e = rc + nn;
  const uint32_t b = s1_ring_batch(ring, p);
  return S1RingSlot{b, p - b * ring, e - s1_ring_batch(ring, e) * ring};
}

// Exhaustive check for one ring size: every rc in [0, ring), every nn in
// [0, S1_TILE_ROWS].  Every rank gets exactly one (batch, slot) with
// slot < ring; the rows carried in (slots 0 .. rc - 1 of batch 0) and the
// ranks never share a slot of a batch; every batch but the last is full when
// it is re-scored; the last one is the new fill, below ring.
constexpr bool s1_ring_check(uint32_t ring) {
  if (S1_TILE_ROWS > 2u * ring) return false;
  for (uint32_t rc = 0; rc < ring; ++rc)
    for (uint32_t nn = 0; nn <= S1_TILE_ROWS; ++nn) {
      uint32_t fill[S1_RING_MAX_FULL + 1] = {rc, 0u, 0u};      // rows per batch
      uint32_t used[S1_RING_MAX_FULL + 1] = {(1u << rc) - 1u, 0u, 0u};  // slots taken per batch
      const S1RingSlot end = s1_ring_slot(ring, rc, nn, nn);
      if (end.batch > S1_RING_MAX_FULL) return false;
      for (uint32_t rk = 0; rk < nn; ++rk) {
        const S1RingSlot r = s1_ring_slot(ring, rc, nn, rk);
        if (r.batch > end.batch || r.slot >= ring) return false;
        if (used[r.batch] & (1u << r.slot)) return false;       // distinct slots within a batch
        // ranks fill a batch in order, and only after the one before it is full
        if (r.slot != fill[r.batch]) return false;
        if (r.batch > 0u && fill[r.batch - 1u] != ring) return false;
        if (r.rc != end.rc) return false;
        used[r.batch] |= 1u << r.slot;
        fill[r.batch] += 1u;
      }
      for (uint32_t b = 0; b < end.batch; ++b)
        if (fill[b] != ring) return false;                       // every batch but the last is full
      if (fill[end.batch] != end.slot || end.rc != end.slot) return false;
      if (end.rc >= ring) return false;                          // the invariant between tiles
      uint32_t total = 0;
      for (uint32_t b = 0; b <= S1_RING_MAX_FULL; ++b) total += fill[b];
      if (total != rc + nn) return false;                        // no row lost, none twice
    }
  return true;
}

static_assert(s1_ring_check(12), "k_s1 re-scoring ring: slot arithmetic broken for the 12-slot ring");
static_assert(s1_ring_check(16), "k_s1 re-scoring ring: slot arithmetic broken for the 16-slot ring");

}  // namespace km
