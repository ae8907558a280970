// collide.hip -- binary Coulomb collisions (Takizuka & Abe 1977) of the particles of one species, or of two, cell by cell
// (vpic_hip_collide; include/vpic_hip.h states the pairing rule and the arithmetic operation by operation, and is the
// authority: tests/collide_ref.py restates it in numpy and tests/test_gpu_collide.py compares every word).
//   1  collide_check_particles / collide_check_cells   the checking pass: every particle inside the range of its own voxel,
//      no dead slot, the starts a partition of the array; the fullest cell
//   2  (the host, policy.h: plan_collide)              sorts a species whose ranges are not exact and checks again; refuses a
//      cell over the cap before anything is written; picks the instance
//   3  collide_kernel<T, SAME, REL>                     ONE CELL PER WORKGROUP AT A TIME (a workgroup takes every
//      gridDim.x-th cell).  T = 64: a workgroup of one wavefront, lane =
//      particle, keys in registers and ranked with cross-lane reads; T = 256: the keys of the cell in LDS, ranked by counting
//      there.  Both stage the cell's momenta and weights in LDS, apply the pairs there and write the momenta back.
// Pairs that share a particle must be applied in order: the triple of an odd cell by one thread, one after the other, and
// between two species every S particle's pairs j, j + n_S, ... by the ONE thread that owns that S particle, in ascending j
// -- the "rounds" of the unequal pairing are that thread's loop, so no barrier separates them and no two threads ever write
// the same particle (an L particle is in exactly one pair).
// REL = true is vpic_hip_collide_relativistic: the same kernel around another pair function (collide_pair_rel, in double).
#include "engine.h"
#include <algorithm>

namespace vpichip {

// device words of a call (Engine::collide_dev): the checking pass's flag and the fullest cell per species; then COLLIDE_SLOTS
// slots of four counters -- cells with a pair, pairs scattered, pairs skipped, one-sided updates -- of which a workgroup adds
// to slot (its number mod COLLIDE_SLOTS), once, when it has done all its cells (measured: one add per CELL to one word took
// 20 of a call's 26 ms at 2 M cells; adds to one address are served one after the other), and the host sums the slots
enum { CW_BAD = 0, CW_FULLEST_A, CW_FULLEST_B, CW_SLOTS = 8, COLLIDE_SLOTS = 64, COLLIDE_WORDS = CW_SLOTS + 4 * COLLIDE_SLOTS };
enum { CS_CELLS = 0, CS_PAIRS, CS_SKIPPED, CS_ONE_SIDED };
// workgroups of a launch at the most: each takes every gridDim.x-th cell (a wavefront per cell: 64 to a CU's 32 slots, twice over)
constexpr int COLLIDE_MAX_GROUPS_WAVE = 16384, COLLIDE_MAX_GROUPS = 4096;
constexpr int COLLIDE_SLAB_ARRAYS = 6;      // ux, uy, uz, w, key, perm: LDS words per particle of a cell

__device__ __forceinline__ unsigned c_mix32(unsigned x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
__device__ __forceinline__ float c_unit(unsigned r) { return ((float)(r >> 8) + 0.5f) * (1.f / 16777216.f); }

struct CollideSpK {
  float *ux, *uy, *uz; const float *q; const float4 *r; const int *starts;
  int order, np;                     // order: 0 nothing to pair, 1 starts = partition[voxel], 2 starts = tpart[tile key]
  float wq, f;                       // f = m_ab / m of this species (the relativistic model: m itself)
  unsigned id;
};
struct CollideK {
  CollideSpK a, b;
  float cvar, dt, den;               // den = (V * m_ab) * m_ab (the relativistic model: V)
  unsigned seed, call, rank;
  const float *draws;                // test mode: 4 floats per particle index, or null
  unsigned long long *words;
  int nx, ny, nz, sy, sz, nv, stride;   // stride: particles of a cell the LDS slab holds, per species
  TileK tk;
};

// ---- the checking pass ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void collide_check_particles(CollideSpK s, CollideK k) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (p < s.np) {
    const int v = record_cell(s.r, p);
    if (v < 0 || v >= k.nv) bad = true;                       // a dead slot, or no voxel at all
    else {
      int cx, cy, cz;
      voxel_cell(v, k.tk, cx, cy, cz);
      if (cx < 1 || cx > k.nx || cy < 1 || cy > k.ny || cz < 1 || cz > k.nz) bad = true;   // a ghost voxel: its cell is never a workgroup's
      else {
        const int at = s.order == 2 ? sort_key<true>(v, k.tk) : v;
        bad = !(p >= s.starts[at] && p < s.starts[at + 1]);
      }
    }
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(k.words + CW_BAD, 1ull);
}
// n_ranges ranges: starts[] ascending from 0 to np; the fullest range into words[slot]
__global__ __launch_bounds__(256) void collide_check_cells(CollideSpK s, int n_ranges, unsigned long long *words, int slot) {
  const int at = blockIdx.x * 256 + threadIdx.x;
  int n = 0; bool bad = false;
  if (at < n_ranges) {
    n = s.starts[at + 1] - s.starts[at];
    bad = n < 0 || (at == 0 && s.starts[0] != 0) || (at == n_ranges - 1 && s.starts[n_ranges] != s.np);
    if (n < 0) n = 0;
  }
  for (int off = 32; off; off >>= 1) n = max(n, __shfl_xor(n, off));
  if ((threadIdx.x & 63) == 0 && n > 0) atomicMax(words + slot, (unsigned long long)n);
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(words + CW_BAD, 1ull);
}

// ---- one cell ------------------------------------------------------------------------------------------------------------
struct Slab { float *ux, *uy, *uz, *w; unsigned *key; int *perm; };
__device__ __forceinline__ Slab slab_at(unsigned *base, int stride) {
  Slab s;
  s.ux = reinterpret_cast<float *>(base); s.uy = s.ux + stride; s.uz = s.uy + stride; s.w = s.uz + stride;
  s.key = base + 4 * stride; s.perm = reinterpret_cast<int *>(base + 5 * stride);
  return s;
}
__device__ __forceinline__ unsigned cell_c0(const CollideK &k, unsigned species, int v) {
  return c_mix32((k.seed ^ c_mix32(k.call * 0x9e3779b9u + species)) + c_mix32(k.rank * 0x85ebca6bu + (unsigned)v));
}
__device__ __forceinline__ void cell_range(const CollideSpK &s, int v, int key, int &lo, int &n) {
  lo = 0; n = 0;
  if (s.order == 0) return;
  const int at = s.order == 2 ? key : v;
  lo = s.starts[at]; n = s.starts[at + 1] - lo;
}
// the cell of workgroup b: by tile key when species a is in tile order (its ranges are then walked in the order of its
// array), else the interior cells in voxel order; false: a cell of a partial tile that lies beyond the grid
__device__ __forceinline__ bool block_cell(const CollideK &k, unsigned b, int &v, int &key) {
  int x, y, z;
  if (k.a.order == 2) {
    const int tile = (int)(b >> 6), c = (int)(b & 63u);
    const int tx = tile % k.tk.ntx, ty = (tile / k.tk.ntx) % k.tk.nty, tz = tile / (k.tk.ntx * k.tk.nty);
    x = tx << 2 | (c & 3); y = ty << 2 | (c >> 2 & 3); z = tz << 2 | (c >> 4);
    if (x >= k.nx || y >= k.ny || z >= k.nz) return false;
  } else {
    x = (int)(b % (unsigned)k.nx); y = (int)((b / (unsigned)k.nx) % (unsigned)k.ny); z = (int)(b / ((unsigned)k.nx * (unsigned)k.ny));
  }
  v = (x + 1) + k.sy * (y + 1) + k.sz * (z + 1);
  key = (((z >> 2) * k.tk.nty + (y >> 2)) * k.tk.ntx + (x >> 2)) * TILE_CELLS + ((z & 3) << 4 | (y & 3) << 2 | (x & 3));
  return true;
}
template <int T>
__device__ __forceinline__ void load_cell(const CollideSpK &s, const Slab &l, int lo, int n, unsigned c0) {
  for (int k = threadIdx.x; k < n; k += T) {
    l.ux[k] = s.ux[lo + k]; l.uy[k] = s.uy[lo + k]; l.uz[k] = s.uz[lo + k];
    l.w[k] = fabsf(s.q[lo + k]) * s.wq;
    l.key[k] = c_mix32(c0 + (unsigned)k);
  }
}
template <int T>
__device__ __forceinline__ void store_cell(const CollideSpK &s, const Slab &l, int lo, int n) {
  for (int k = threadIdx.x; k < n; k += T) { s.ux[lo + k] = l.ux[k]; s.uy[lo + k] = l.uy[k]; s.uz[lo + k] = l.uz[k]; }
}
// perm[r] = the k whose key is the r-th smallest.  T == 64 (n <= 64): lane k holds key k and counts the smaller ones with
// cross-lane reads; T == 256: every thread counts, for each of its k, the smaller keys in LDS (all lanes read the same word
// at a time: a broadcast, no bank conflict)
template <int T>
__device__ __forceinline__ void rank_cell(const Slab &l, int n, unsigned c0) {
  if (T == 64) {
    const unsigned mine = c_mix32(c0 + threadIdx.x);
    int r = 0;
    for (int j = 0; j < n; j++) r += (unsigned)__shfl((int)mine, j) < mine ? 1 : 0;
    if ((int)threadIdx.x < n) l.perm[r] = (int)threadIdx.x;
  } else {
    for (int k = threadIdx.x; k < n; k += T) {
      const unsigned mine = l.key[k];
      int r = 0;
      for (int j = 0; j < n; j++) r += l.key[j] < mine ? 1 : 0;
      l.perm[r] = k;
    }
  }
}

struct Draws { float n, c, s, u; };
__device__ __forceinline__ Draws pair_draws(const CollideK &k, unsigned c0, unsigned j, int first_index) {
  Draws d;
  if (k.draws) {
    const float4 t = reinterpret_cast<const float4 *>(k.draws)[first_index];
    d.n = t.x; d.c = t.y; d.s = t.z; d.u = t.w;
  } else {
    const unsigned base = c_mix32(c0 ^ 0x2545f491u) + 4u * j;
    const float u0 = c_unit(c_mix32(base)), u1 = c_unit(c_mix32(base + 1u)), u2 = c_unit(c_mix32(base + 2u));
    // (cospif / sinpif: the reduction of a multiple of pi is exact)
    d.n = sqrtf(-2.f * logf(u0)) * cospif(2.f * u1);
    d.s = sinpif(2.f * u2); d.c = cospif(2.f * u2);
    d.u = c_unit(c_mix32(base + 3u));
  }
  return d;
}
// one pair, include/vpic_hip.h operation by operation (no contraction: -ffp-contract=off; / and sqrtf correctly rounded).
// F and S may be the same slab (one species): kf != ks always.  Returns PAIR_*: skipped (gm == 0), scattered, or
// scattered with not both particles updated.
enum { PAIR_SKIPPED = 0, PAIR_SCATTERED = 1, PAIR_ONE_SIDED = 2 };
__device__ __forceinline__ int collide_pair(const CollideK &k, const Slab &F, int kf, const Slab &S, int ks, float ff, float fs, float fN, bool half,
                                            const Draws &d) {
  const float gx = F.ux[kf] - S.ux[ks], gy = F.uy[kf] - S.uy[ks], gz = F.uz[kf] - S.uz[ks];
  const float gq = gx * gx + gy * gy, g2 = gq + gz * gz, gm = sqrtf(g2), gp = sqrtf(gq);
  if (gm == 0.f) return PAIR_SKIPPED;
  const float wf = F.w[kf], ws = S.w[ks];
  float s2 = (((k.cvar * fmaxf(wf, ws)) * fN) * k.dt) / (k.den * ((gm * gm) * gm));
  if (half) s2 = 0.5f * s2;
  const float dl = d.n * sqrtf(s2), t = dl * dl;
  float sin_t = 0.f, omc = 2.f;
  if (t < 18446744073709551616.f) { sin_t = (2.f * dl) / (1.f + t); omc = (2.f * t) / (1.f + t); }
  const float sc = sin_t * d.c, ss = sin_t * d.s;
  float Dx, Dy, Dz;
  if (gp != 0.f) {
    const float ax = gx / gp, ay = gy / gp;
    Dx = ((ax * gz) * sc - (ay * gm) * ss) - gx * omc;
    Dy = ((ay * gz) * sc + (ax * gm) * ss) - gy * omc;
    Dz = (-(gp * sc)) - gz * omc;
  } else { Dx = gm * sc; Dy = gm * ss; Dz = -(gz * omc); }
  const bool do_f = ws >= wf || d.u * wf < ws, do_s = wf >= ws || d.u * ws < wf;
  if (do_f) { F.ux[kf] = F.ux[kf] + ff * Dx; F.uy[kf] = F.uy[kf] + ff * Dy; F.uz[kf] = F.uz[kf] + ff * Dz; }
  if (do_s) { S.ux[ks] = S.ux[ks] - fs * Dx; S.uy[ks] = S.uy[ks] - fs * Dy; S.uz[ks] = S.uz[ks] - fs * Dz; }
  return do_f && do_s ? PAIR_SCATTERED : PAIR_ONE_SIDED;
}

// one pair of vpic_hip_collide_relativistic (Perez et al. 2012), include/vpic_hip.h operation by operation: the float momenta,
// masses, weights and draws promoted to double, every operation in double (unfused; / and sqrt correctly rounded), the two new
// momenta rounded to float once each.  mf, ms: the masses of the pair's first and second particle; k.den is V here.  gamma
// is computed from the slab's momenta of this moment: an S particle's change between its pairs.
__device__ __forceinline__ int collide_pair_rel(const CollideK &k, const Slab &F, int kf, const Slab &S, int ks, float mf_, float ms_, float fN, bool half,
                                                const Draws &d) {
  const float fx = F.ux[kf], fy = F.uy[kf], fz = F.uz[kf], sx = S.ux[ks], sy = S.uy[ks], sz = S.uz[ks];
  if (fx == sx && fy == sy && fz == sz) return PAIR_SKIPPED;
  const double ufx = fx, ufy = fy, ufz = fz, usx = sx, usy = sy, usz = sz, mf = mf_, ms = ms_;
  const double gf = sqrt(1.0 + ((ufx * ufx + ufy * ufy) + ufz * ufz)), gs = sqrt(1.0 + ((usx * usx + usy * usy) + usz * usz));
  const double ef = mf * gf, es = ms * gs, E = ef + es, rE = 1.0 / E;
  const double vx = (mf * ufx + ms * usx) * rE, vy = (mf * ufy + ms * usy) * rE, vz = (mf * ufz + ms * usz) * rE;
  const double gC = 1.0 / sqrt(1.0 - ((vx * vx + vy * vy) + vz * vz)), kC = (gC * gC) / (gC + 1.0);
  const double vuf = (vx * ufx + vy * ufy) + vz * ufz, vus = (vx * usx + vy * usy) + vz * usz;
  const double cf = kC * vuf - gC * gf;
  const double px = mf * (ufx + cf * vx), py = mf * (ufy + cf * vy), pz = mf * (ufz + cf * vz);
  const double esf = mf * (gC * (gf - vuf)), ess = ms * (gC * (gs - vus));          // m gamma* of each in the pair's frame
  const double pq = px * px + py * py, p2 = pq + pz * pz, pm = sqrt(p2), gp = sqrt(pq);
  if (pm == 0.0) return PAIR_SKIPPED;
  const float wf = F.w[kf], ws = S.w[ks];
  const double r = (esf * ess) / (pm * pm) + 1.0;
  double s2 = (((((double)k.cvar * (double)fmaxf(wf, ws)) * (double)fN) * (double)k.dt) * (((gC * pm) * rE) * (r * r))) / ((double)k.den * (ef * es));
  if (half) s2 = 0.5 * s2;
  const double dl = (double)d.n * sqrt(s2), t = dl * dl;
  double sin_t = 0.0, omc = 2.0;
  if (t < 18446744073709551616.0) { sin_t = (2.0 * dl) / (1.0 + t); omc = (2.0 * t) / (1.0 + t); }
  const double sc = sin_t * (double)d.c, ss = sin_t * (double)d.s;
  double Dx, Dy, Dz;
  if (gp != 0.0) {
    const double ax = px / gp, ay = py / gp;
    Dx = ((ax * pz) * sc - (ay * pm) * ss) - px * omc;
    Dy = ((ay * pz) * sc + (ax * pm) * ss) - py * omc;
    Dz = (-(gp * sc)) - pz * omc;
  } else { Dx = pm * sc; Dy = pm * ss; Dz = -(pz * omc); }
  const double qx = px + Dx, qy = py + Dy, qz = pz + Dz;
  const double kvq = kC * ((vx * qx + vy * qy) + vz * qz);
  const bool do_f = ws >= wf || d.u * wf < ws, do_s = wf >= ws || d.u * ws < wf;
  if (do_f) {
    const double a = kvq + esf * gC, rm = 1.0 / mf;
    F.ux[kf] = (float)((qx + vx * a) * rm); F.uy[kf] = (float)((qy + vy * a) * rm); F.uz[kf] = (float)((qz + vz * a) * rm);
  }
  if (do_s) {
    const double a = ess * gC - kvq, rm = 1.0 / ms;
    S.ux[ks] = (float)((vx * a - qx) * rm); S.uy[ks] = (float)((vy * a - qy) * rm); S.uz[ks] = (float)((vz * a - qz) * rm);
  }
  return do_f && do_s ? PAIR_SCATTERED : PAIR_ONE_SIDED;
}
// the pair of a kernel instance: ff, fs are m_ab / m of the two particles (REL: their masses)
template <bool REL>
__device__ __forceinline__ int pair_of(const CollideK &k, const Slab &F, int kf, const Slab &S, int ks, float ff, float fs, float fN, bool half, const Draws &d) {
  return REL ? collide_pair_rel(k, F, kf, S, ks, ff, fs, fN, half, d) : collide_pair(k, F, kf, S, ks, ff, fs, fN, half, d);
}

extern __shared__ unsigned collide_lds[];
template <int T, bool SAME, bool REL>
__global__ __launch_bounds__(T) void collide_kernel(CollideK k, unsigned n_cells) {
  __shared__ unsigned s_cnt[3];
  const Slab A = slab_at(collide_lds, k.stride), B = slab_at(collide_lds + (SAME ? 0 : COLLIDE_SLAB_ARRAYS * k.stride), k.stride);
  if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
  unsigned n_pairs = 0, n_skipped = 0, n_one_sided = 0, cells = 0;
  const auto count = [&](int what) { n_skipped += what == PAIR_SKIPPED; n_pairs += what != PAIR_SKIPPED; n_one_sided += what == PAIR_ONE_SIDED; };
  // (every `continue` below is taken by the whole workgroup: the barriers stay aligned.  A slab word is loaded and stored by
  // the same thread for every cell, and perm[] / key[] of the next cell are written behind that cell's first barrier, which
  // every thread reaches after it has left this cell's pairs: no barrier is needed between two cells.)
  for (unsigned cell = blockIdx.x; cell < n_cells; cell += gridDim.x) {
    int v, key;
    if (!block_cell(k, cell, v, key)) continue;
    int lo_a, n_a, lo_b = 0, n_b = 0;
    cell_range(k.a, v, key, lo_a, n_a);
    if (!SAME) cell_range(k.b, v, key, lo_b, n_b);
    if (SAME ? n_a < 2 : (n_a < 1 || n_b < 1)) continue;
    if (n_a > k.stride || n_b > k.stride || lo_a < 0 || lo_b < 0 || lo_a + n_a > k.a.np || (!SAME && lo_b + n_b > k.b.np)) continue;   // (the host has refused such a call: never index beyond the slab or the array)
    cells++;
    const unsigned c0_a = cell_c0(k, k.a.id, v), c0_b = cell_c0(k, k.b.id, v);
    load_cell<T>(k.a, A, lo_a, n_a, c0_a);
    if (!SAME) load_cell<T>(k.b, B, lo_b, n_b, c0_b);
    __syncthreads();
    rank_cell<T>(A, n_a, c0_a);
    if (!SAME) rank_cell<T>(B, n_b, c0_b);
    __syncthreads();
    if (SAME) {
      const int n = n_a;
      const float fN = (float)n;
      if (n & 1) {
        if (threadIdx.x == T - 1) {            // the triple, one pair after the other, each at half the variance
          const int p0 = A.perm[0], p1 = A.perm[1], p2 = A.perm[2];
          count(pair_of<REL>(k, A, p0, A, p1, k.a.f, k.a.f, fN, true, pair_draws(k, c0_a, 0u, lo_a + p0)));
          count(pair_of<REL>(k, A, p1, A, p2, k.a.f, k.a.f, fN, true, pair_draws(k, c0_a, 1u, lo_a + p1)));
          count(pair_of<REL>(k, A, p2, A, p0, k.a.f, k.a.f, fN, true, pair_draws(k, c0_a, 2u, lo_a + p2)));
        }
        for (int m = threadIdx.x; m < (n - 3) / 2; m += T) {
          const int kf = A.perm[3 + 2 * m], ks = A.perm[4 + 2 * m];
          count(pair_of<REL>(k, A, kf, A, ks, k.a.f, k.a.f, fN, false, pair_draws(k, c0_a, (unsigned)(3 + m), lo_a + kf)));
        }
      } else {
        for (int j = threadIdx.x; j < n / 2; j += T) {
          const int kf = A.perm[2 * j], ks = A.perm[2 * j + 1];
          count(pair_of<REL>(k, A, kf, A, ks, k.a.f, k.a.f, fN, false, pair_draws(k, c0_a, (unsigned)j, lo_a + kf)));
        }
      }
    } else {
      const bool swap = n_b > n_a;               // L: the species with more particles here, a on a tie
      const Slab &L = swap ? B : A, &S = swap ? A : B;
      const int n_L = swap ? n_b : n_a, n_S = swap ? n_a : n_b, lo_L = swap ? lo_b : lo_a;
      const float f_L = swap ? k.b.f : k.a.f, f_S = swap ? k.a.f : k.b.f, fN = (float)n_S;
      const unsigned c0_L = swap ? c0_b : c0_a;
      for (int m = threadIdx.x; m < n_S; m += T) {
        const int ks = S.perm[m];
        for (int j = m; j < n_L; j += n_S) {     // this S particle's pairs, in ascending j
          const int kf = L.perm[j];
          count(pair_of<REL>(k, L, kf, S, ks, f_L, f_S, fN, false, pair_draws(k, c0_L, (unsigned)j, lo_L + kf)));
        }
      }
    }
    __syncthreads();
    store_cell<T>(k.a, A, lo_a, n_a);
    if (!SAME) store_cell<T>(k.b, B, lo_b, n_b);
  }
  __syncthreads();                               // (s_cnt is zero for everybody, also in a workgroup that had no cell)
  if (n_pairs) atomicAdd(&s_cnt[0], n_pairs);
  if (n_skipped) atomicAdd(&s_cnt[1], n_skipped);
  if (n_one_sided) atomicAdd(&s_cnt[2], n_one_sided);
  __syncthreads();
  if (threadIdx.x == 0 && cells) {
    unsigned long long *slot = k.words + CW_SLOTS + 4 * (blockIdx.x % COLLIDE_SLOTS);
    atomicAdd(slot + CS_CELLS, (unsigned long long)cells);
    if (s_cnt[0]) atomicAdd(slot + CS_PAIRS, (unsigned long long)s_cnt[0]);
    if (s_cnt[1]) atomicAdd(slot + CS_SKIPPED, (unsigned long long)s_cnt[1]);
    if (s_cnt[2]) atomicAdd(slot + CS_ONE_SIDED, (unsigned long long)s_cnt[2]);
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
static CollideSpecies describe(const Species &s, const TileK &tk) {
  CollideSpecies d;
  d.np = s.np; d.n_sorted = s.n_sorted; d.n_holes = s.n_holes; d.fuse_pending = s.fuse_pending;
  d.tile_valid = s.tile_valid && tile_partition_usable(s, tk); d.coarse_sorted = s.coarse_sorted;
  d.partition_valid = !s.tile_valid && s.partition_valid && s.partition;
  return d;
}
static CollideSpK species_k(const Species &s, const CollideSpecies &d, int id, float wq, float f) {
  CollideSpK k;
  k.ux = s.p.ux; k.uy = s.p.uy; k.uz = s.p.uz; k.q = s.p.q; k.r = s.p.r;
  k.order = s.np == 0 ? 0 : d.tile_valid ? 2 : 1;
  k.starts = k.order == 2 ? s.tpart : s.partition;
  k.np = (int)s.np; k.wq = wq; k.f = f; k.id = (unsigned)id;
  return k;
}
// a species whose ranges are not exact: sorted in the order it is in (or, in none, the one a sort would give it now), by cell
static int sort_exact(Engine *e, Species &s, bool wants_tile) {
  if (s.nm > 0) VH_FAIL("collide: the species must be sorted first and has %lld movers pending", (long long)s.nm);
  const bool tile = s.tile_valid || (!s.partition_valid && wants_tile);
  const int knob = e->knobs.tile_coarse;
  e->knobs.tile_coarse = 0;                    // never by tile only (plan_sort: the knob overrules the policy), whatever the environment says
  const int rc = k_sort_p(e, s, tile, false);  // (a sort pending inside the push -- fuse_pending -- is dropped by this plain one)
  e->knobs.tile_coarse = knob;
  return rc;
}
static int check_species(Engine *e, const CollideSpK &s, const CollideK &k, int slot) {
  if (s.order == 0) return 0;
  const int n_ranges = s.order == 2 ? k.tk.ntiles * TILE_CELLS : k.nv;
  hipLaunchKernelGGL(collide_check_cells, dim3((n_ranges + 255) / 256), dim3(256), 0, e->stream, s, n_ranges, k.words, slot);
  hipLaunchKernelGGL(collide_check_particles, dim3((s.np + 255) / 256), dim3(256), 0, e->stream, s, k);
  VH_CHECK(hipGetLastError());
  return 0;
}

template <bool REL>
static void launch_collide(Engine *e, const CollideK &K, bool wave, bool same, unsigned groups, size_t lds, unsigned cells) {
  if (wave) {
    if (same) hipLaunchKernelGGL((collide_kernel<64, true, REL>), dim3(groups), dim3(64), lds, e->stream, K, cells);
    else hipLaunchKernelGGL((collide_kernel<64, false, REL>), dim3(groups), dim3(64), lds, e->stream, K, cells);
  } else {
    if (same) hipLaunchKernelGGL((collide_kernel<256, true, REL>), dim3(groups), dim3(256), lds, e->stream, K, cells);
    else hipLaunchKernelGGL((collide_kernel<256, false, REL>), dim3(groups), dim3(256), lds, e->stream, K, cells);
  }
}

int k_collide(Engine *e, const vpic_hip_collision_t &c, bool wants_tile_a, bool wants_tile_b, bool relativistic) {
  for (auto &w : e->collide_last) w = 0;
  e->collide_instance = 0;
  if (!e->collide_dev) VH_CHECK(hipMalloc((void **)&e->collide_dev, COLLIDE_WORDS * sizeof(unsigned long long)));
  if (!e->collide_host) VH_CHECK(hipHostMalloc((void **)&e->collide_host, COLLIDE_WORDS * sizeof(unsigned long long), hipHostMallocDefault));
  Species &A = e->species[c.sp_a], &B = e->species[c.sp_b];
  const bool same = c.sp_a == c.sp_b;
  const float m_b = same ? c.m_a : c.m_b, wq_b = same ? c.wq_a : c.wq_b;
  const float m_ab = (c.m_a * m_b) / (c.m_a + m_b);
  const float V = (e->grid.dx * e->grid.dy) * e->grid.dz;
  CollideK K;
  K.cvar = c.cvar; K.dt = c.dt; K.den = relativistic ? V : (V * m_ab) * m_ab;
  K.seed = c.seed; K.call = c.call; K.rank = (unsigned)e->gk.rank;
  K.draws = e->collide_draws_n > 0 ? e->collide_draws : nullptr;
  K.words = e->collide_dev;
  K.nx = e->gk.nx; K.ny = e->gk.ny; K.nz = e->gk.nz; K.sy = e->gk.sy; K.sz = e->gk.sz; K.nv = e->gk.nv; K.stride = 0;
  K.tk = make_tile_k(e->gk);
  CollideSpecies da = describe(A, K.tk), db = describe(B, K.tk);
  CollidePlan pl;
  bool checked = false, sorted = false;
  for (int round = 0;; round++) {
    pl = plan_collide(da, db, same, VPIC_HIP_COLLIDE_MAX_CELL, e->knobs.collide_group);
    if (!pl.sort_a && !pl.sort_b && checked) break;
    if (round == 2) VH_FAIL("collide: the cell ranges of a species are not exact after a sort (a particle in a ghost voxel?)");
    if (pl.sort_a) { if (sort_exact(e, A, wants_tile_a)) return 1; sorted = true; }
    if (pl.sort_b) { if (sort_exact(e, B, wants_tile_b)) return 1; sorted = true; }
    da = describe(A, K.tk); db = describe(B, K.tk);
    K.a = species_k(A, da, c.sp_a, c.wq_a, relativistic ? c.m_a : m_ab / c.m_a);
    K.b = species_k(B, db, c.sp_b, wq_b, relativistic ? m_b : m_ab / m_b);
    // (a species that is still not in a sorted order -- it holds nothing alive -- has no ranges to check)
    if (A.np > 0 && !da.tile_valid && !da.partition_valid) VH_FAIL("collide: species %d could not be sorted", c.sp_a);
    if (!same && B.np > 0 && !db.tile_valid && !db.partition_valid) VH_FAIL("collide: species %d could not be sorted", c.sp_b);
    VH_CHECK(hipMemsetAsync(e->collide_dev, 0, COLLIDE_WORDS * sizeof(unsigned long long), e->stream));
    if (check_species(e, K.a, K, CW_FULLEST_A)) return 1;
    if (!same && check_species(e, K.b, K, CW_FULLEST_B)) return 1;
    VH_CHECK(hipMemcpyAsync(e->collide_host, e->collide_dev, COLLIDE_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    VH_CHECK(hipStreamSynchronize(e->stream));
    // (one flag for both species: where it is set, both are sorted again)
    da.check_failed = db.check_failed = e->collide_host[CW_BAD] != 0;
    da.fullest = (int64_t)e->collide_host[CW_FULLEST_A]; db.fullest = (int64_t)e->collide_host[CW_FULLEST_B];
    checked = true;
  }
  const int64_t fullest = same ? da.fullest : std::max(da.fullest, db.fullest);
  e->collide_last[4] = fullest; e->collide_last[5] = sorted ? 1 : 0;
  if (pl.over_cap) VH_FAIL("collide: a cell holds %lld particles of one species, VPIC_HIP_COLLIDE_MAX_CELL is %d", (long long)fullest, VPIC_HIP_COLLIDE_MAX_CELL);
  if (pl.instance == CollideInstance::none) return 0;
  const bool wave = pl.instance == CollideInstance::wave;
  K.stride = wave ? COLLIDE_WAVE_CELL : (int)((fullest + 63) / 64 * 64);
  const size_t lds = sizeof(unsigned) * COLLIDE_SLAB_ARRAYS * (size_t)K.stride * (same ? 1 : 2);
  const unsigned cells = K.a.order == 2 ? (unsigned)(K.tk.ntiles * TILE_CELLS) : (unsigned)(K.nx * K.ny * K.nz);
  const unsigned groups = std::min(cells, (unsigned)(wave ? COLLIDE_MAX_GROUPS_WAVE : COLLIDE_MAX_GROUPS));
  if (relativistic) launch_collide<true>(e, K, wave, same, groups, lds, cells);
  else launch_collide<false>(e, K, wave, same, groups, lds, cells);
  VH_CHECK(hipGetLastError());
  e->collide_instance = wave ? 1 : 2;
  VH_CHECK(hipMemcpyAsync(e->collide_host, e->collide_dev, COLLIDE_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
  VH_CHECK(hipStreamSynchronize(e->stream));
  for (int slot = 0; slot < COLLIDE_SLOTS; slot++)
    for (int w = 0; w < 4; w++) e->collide_last[w] += (int64_t)e->collide_host[CW_SLOTS + 4 * slot + w];
  return 0;
}

}  // namespace vpichip
