// particle_match.h -- the row of a particle in a tile of rows of another frame: an open-addressing
// table particle -> row in LDS that keeps the lowest row of a repeated particle, with bounded probe
// loops (drift: drift_kernels.h; two-point correlations: twopoint_kernels.h).  Included
// inside the anonymous namespace of a unit.  A tile holds at most DR_TILE rows, so the table is never
// more than half full and a probe always meets an empty slot or its particle.
#ifndef CTREFINE_PARTICLE_MATCH_H
#define CTREFINE_PARTICLE_MATCH_H

constexpr int DR_TILE = 2048;           // rows of the other frame in one LDS table
constexpr int DR_SLOTS = 4096;          // its slots, 8 bytes each: never more than half full
constexpr unsigned long long DR_EMPTY = ~0ull;

__device__ __forceinline__ unsigned drift_slot(int p) { return ((unsigned)p * 2654435761u) >> 20; }   // 12 bits: DR_SLOTS

// (particle << 32 | row) into the table; a particle that is there already keeps the lower row
__device__ __forceinline__ void drift_insert(unsigned long long* tab, int p, unsigned row) {
  const unsigned long long mine = ((unsigned long long)(unsigned)p << 32) | row;
  unsigned s = drift_slot(p);
  for (int probe = 0; probe < DR_SLOTS; ++probe, s = (s + 1) & (DR_SLOTS - 1)) {
    const unsigned long long old = atomicCAS(tab + s, DR_EMPTY, mine);
    if (old == DR_EMPTY) return;
    if ((unsigned)(old >> 32) == (unsigned)p) { atomicMin(tab + s, mine); return; }
  }
}

// the row of particle p in the table, or -1
__device__ __forceinline__ int drift_lookup(const unsigned long long* tab, int p) {
  unsigned s = drift_slot(p);
  for (int probe = 0; probe < DR_SLOTS; ++probe, s = (s + 1) & (DR_SLOTS - 1)) {
    const unsigned long long v = tab[s];
    if (v == DR_EMPTY) return -1;
    if ((unsigned)(v >> 32) == (unsigned)p) return (int)(unsigned)v;
  }
  return -1;
}

#endif  // CTREFINE_PARTICLE_MATCH_H
