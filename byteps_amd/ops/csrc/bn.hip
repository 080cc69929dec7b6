// Fused BatchNorm(+residual)(+ReLU) training kernels for gfx950 — NHWC
// (channels_last) bf16 with fp32 statistics.
//
// Replaces MIOpen's 3-kernel fwd + 3-kernel bwd spatial batchnorm, which
// profiling showed at ~30% of a ResNet-50 bf16 step on MI355X
// (profiles/resnet50_steady_state.md).  Design per the CDNA4 guide:
// memory-bound single-pass kernels, 8×bf16 (16 B) vector accesses on the
// fastest (channel) dimension, fp32 accumulation.  Two launches per
// direction: a statistics kernel that folds its per-block partials inside
// the launch, then an apply kernel.
//
// Layout: x is [M, C] row-major with C contiguous (NHWC), M = N*H*W.
// Requires C % 8 == 0 and C <= 2048 (python falls back to torch
// otherwise).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define BLOCK 256
#define MAX_GRID 2048

namespace {

using bf16 = __hip_bfloat16;
typedef short short8 __attribute__((ext_vector_type(8)));
typedef float float4v __attribute__((ext_vector_type(4)));

__device__ inline float bf2f(bf16 v) { return __bfloat162float(v); }
__device__ inline bf16 f2bf(float v) { return __float2bfloat16(v); }

struct F8 {
  float v[8];
  __device__ void zero() {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0.0f;
  }
};

__device__ inline void load8(const bf16* p, float* out) {
  short8 r = *reinterpret_cast<const short8*>(p);
  const bf16* e = reinterpret_cast<const bf16*>(&r);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = bf2f(e[i]);
}

__device__ inline void store8(bf16* p, const float* in) {
  short8 r;
  bf16* e = reinterpret_cast<bf16*>(&r);
#pragma unroll
  for (int i = 0; i < 8; ++i) e[i] = f2bf(in[i]);
  *reinterpret_cast<short8*>(p) = r;
}

// ---------------------------------------------------------------------------
// Statistics: one launch per direction.
//
// fwd: x → per-channel Σx, Σx² → mean, invstd, running-stat update.
// bwd: x, dy, mask → sums2[2C] = [Σdz, Σdz·xhat].
//
// Geometry (stat_geom): the grid is R row-blocks × S channel slices.  A
// slice is at most STAT_CS short8 slots (128 channels), so a block's
// partial is at most 2·128 fp32 = 1 KB.  Each thread owns one slot and
// every R·groups-th row, and keeps U independent 16-B loads in flight per
// trip.  R gives each thread one trip where that needs at most
// STAT_TARGET_BLOCKS blocks in all (big tensors loop), no fewer than
// STAT_MIN_BLOCKS blocks while there are rows for them, and at most FOLD_G².
//
// Combine inside the launch, wait-free, by the last arriver: every block
// stores its partial write-through (sc1), drains, and takes a ticket on its
// group's counter.  The block that draws the group's last ticket reads the
// group's ≤ FOLD_G partials (≤ 16 KB) with sc1 loads, folds them in block
// order and, when there is more than one group, does the same once more on
// a per-slice counter over the group totals.  sc1 stores + sc1 loads make
// the hand-off visible across XCDs without an agent release in every block
// (an L2 write-back each) or an acquire in the reducer.  No block ever
// waits on another; the fold order is fixed, so results are bitwise
// reproducible.  Each counter sits on its own 128-B line: agent-scope
// atomics to one line serialise, and a shared line cost several µs.
//
// Counter state: zeroed once when allocated (fused_bn.py) and reset to
// zero by the last arriver, so a launch leaves every counter at zero.
// That avoids a memset node per call, and holds because each launch runs
// to completion before the next one on the same stream starts; the one
// thing it rules out is two launches sharing a counter buffer in flight
// at once (one buffer per module and direction, used on one stream).
// ---------------------------------------------------------------------------

#define STAT_CS 16               // max short8 slots per channel slice
#define STAT_SMAX (2048 / 8 / STAT_CS)
#define FOLD_G 16                // max partials one reducer folds
#define STAT_TARGET_BLOCKS 1024
#define STAT_MIN_BLOCKS 256       // one per CU
#define FWD_U 8                  // rows in flight per thread, fwd
#define BWD_U 4                  // bwd (x + dy + mask byte per row)
#define TICKET_STRIDE 32         // words: one counter per 128-B line
// counter words per direction: [slice][group] then [slice]
#define BN_TICKET_WORDS ((STAT_SMAX * FOLD_G + STAT_SMAX) * TICKET_STRIDE)

typedef __attribute__((address_space(1))) unsigned gu32;

struct StatGeom {
  int cs;  // short8 slots per slice
  int S;   // channel slices (grid.y)
  int R;   // row-blocks per slice (grid.x)
  int G;   // row-blocks per fold group
  int NG;  // fold groups per slice
};

inline StatGeom stat_geom(long long M, int C, int U) {
  StatGeom g;
  const int cpt = C >> 3;
  g.cs = cpt < STAT_CS ? cpt : STAT_CS;
  g.S = (cpt + g.cs - 1) / g.cs;
  const long long groups = BLOCK / g.cs;
  const long long per_iter = groups * U;
  long long R = (M + per_iter - 1) / per_iter;  // one trip per thread
  const long long want = (STAT_TARGET_BLOCKS + g.S - 1) / g.S;
  if (R > want) R = want;
  // small tensors: spread over at least STAT_MIN_BLOCKS blocks (a row
  // group per thread at the least) rather than pack U rows per thread
  const long long floor_r = (STAT_MIN_BLOCKS + g.S - 1) / g.S;
  if (R < floor_r) R = min(floor_r, (M + groups - 1) / groups);
  if (R > FOLD_G * FOLD_G) R = FOLD_G * FOLD_G;
  if (R < 1) R = 1;
  g.R = (int)R;
  g.NG = (g.R + FOLD_G - 1) / FOLD_G;
  g.G = (g.R + g.NG - 1) / g.NG;  // balanced groups, each ≤ FOLD_G
  return g;
}

// fp32 words of partials a launch needs (level-1 then level-2)
inline long long stat_ws_floats(const StatGeom& g) {
  const long long nj = 16LL * g.cs;
  return (long long)g.S * (g.R + g.NG) * nj;
}

__device__ inline void drain_vm() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Take a ticket on `cnt`, which expects `n` arrivals, once this block's
// sc1 partial stores are complete.  Returns (block-uniformly) whether this
// block arrived last; if so the counter is back at zero and the other
// arrivers' partials can be read with sc1 loads (ld_sc1).
__device__ inline bool arrive_last(unsigned* cnt, unsigned n, float* lds,
                                   int flag_slot) {
  drain_vm();          // every storing wave: its sc1 stores have landed
  __syncthreads();
  if (threadIdx.x == 0) {
    gu32* c = (gu32*)cnt;
    const unsigned tk = __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
    const bool last = tk == n - 1;
    if (last) {
      __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // every load of the partials is sc1: no cache invalidate needed, only
      // keep the compiler from moving those loads above the ticket
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    lds[flag_slot] = last ? 1.0f : 0.0f;
  }
  __syncthreads();
  return lds[flag_slot] != 0.0f;
}

// write-through store / L2-bypassing load of a partial (global_*_dword sc1)
__device__ inline void st_sc1(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline float ld_sc1(const float* p) {
  return __hip_atomic_load(const_cast<float*>(p), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// Σ_k src[k*nj], k < n, in k order; loads issued 8 at a time (indices
// clamped rather than branched around, so all 8 are in flight together)
__device__ inline float fold_rows(const float* src, int n, int nj) {
  float acc = 0.0f;
  for (int k0 = 0; k0 < n; k0 += 8) {
    float p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = min(k0 + u, n - 1);
      p[u] = ld_sc1(src + (long long)k * nj);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (k0 + u < n) acc += p[u];
  }
  return acc;
}

// Block partial → two-level fold.  `lds` holds [groups][nj] per-thread
// sums on entry.  Returns true only in the one block per slice that ends
// holding the slice's totals, in lds[0..nj).
__device__ inline bool stat_combine(float* lds, int groups, int nj,
                                    float* ws, unsigned* tickets, int R,
                                    int G, int NG) {
  const int t = threadIdx.x;
  const int slice = blockIdx.y;
  const int rb = blockIdx.x;
  const int flag_slot = BLOCK * 16;
  __syncthreads();
  float v = 0.0f;
  if (t < nj)
    for (int g = 0; g < groups; ++g) v += lds[g * nj + t];

  // level 1: this block's partial, ticket on its group
  float* part1 = ws + (long long)slice * R * nj;
  if (t < nj) st_sc1(part1 + (long long)rb * nj + t, v);
  const int grp = rb / G;
  const int g0 = grp * G;
  const int gn = min(G, R - g0);
  if (!arrive_last(tickets + (slice * FOLD_G + grp) * TICKET_STRIDE, gn,
                   lds, flag_slot))
    return false;
  float acc = 0.0f;
  if (t < nj) acc = fold_rows(part1 + (long long)g0 * nj + t, gn, nj);

  // level 2: group totals, ticket on the slice
  if (NG > 1) {
    float* part2 = ws + (long long)gridDim.y * R * nj +
                   (long long)slice * NG * nj;
    if (t < nj) st_sc1(part2 + (long long)grp * nj + t, acc);
    if (!arrive_last(tickets + (STAT_SMAX * FOLD_G + slice) * TICKET_STRIDE,
                     NG, lds, flag_slot))
      return false;
    if (t < nj) acc = fold_rows(part2 + t, NG, nj);
  }
  if (t < nj) lds[t] = acc;
  __syncthreads();
  return true;
}

// Thread → (row group g, slot c8) within a block's slice.  Rows of one
// thread: g + rb·groups + k·R·groups.
struct StatLane {
  int groups, g, s, c8;
  bool active;
  __device__ StatLane(int cs, int cpt) {
    groups = BLOCK / cs;
    g = threadIdx.x / cs;
    s = threadIdx.x - g * cs;
    c8 = blockIdx.y * cs + s;
    active = g < groups && c8 < cpt;
  }
};

// write a thread's 2×8 sums to lds[g][j] (j = s*8+i, and CSW + s*8+i)
__device__ inline void stat_to_lds(float* lds, const StatLane& L, int cs,
                                   const F8& a, const F8& b) {
  if (L.g >= L.groups) return;
  const int nj = 16 * cs;
  float* row = lds + L.g * nj + L.s * 8;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    row[i] = a.v[i];
    row[8 * cs + i] = b.v[i];
  }
}

template <int U>
__global__ __launch_bounds__(BLOCK) void bn_fwd_stats_kernel(
    const bf16* __restrict__ x, long long M, int C, float eps,
    float momentum, float* __restrict__ mean_out,
    float* __restrict__ invstd_out, float* __restrict__ running_mean,
    float* __restrict__ running_var, int update_running, float* ws,
    unsigned* tickets, int G, int NG) {
  __shared__ float lds[BLOCK * 16 + 1];
  const int cpt = C >> 3;
  const int cs = min(cpt, STAT_CS);
  const int R = gridDim.x;
  const StatLane L(cs, cpt);

  F8 s, q;
  s.zero();
  q.zero();
  if (L.active) {
    const long long stride = (long long)R * L.groups;
    long long row = (long long)blockIdx.x * L.groups + L.g;
    const bf16* xp = x + (L.c8 << 3);
    // rows past M are clamped to the last row and not accumulated, so
    // every trip keeps U loads in flight, the tail included
    for (; row < M; row += U * stride) {
      short8 r[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long rr = min(row + u * stride, M - 1);
        r[u] = *reinterpret_cast<const short8*>(xp + rr * C);
      }
      // keep all U loads issued before the first use (the scheduler
      // otherwise interleaves them with the math, one wait per load)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // a select, not a branch: a branch lets the compiler sink the
        // loads behind it and wait for each one in turn
        const bool in = row + u * stride < M;
        const bf16* e = reinterpret_cast<const bf16*>(&r[u]);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float v = in ? bf2f(e[i]) : 0.0f;
          s.v[i] += v;
          q.v[i] += v * v;
        }
      }
    }
  }
  stat_to_lds(lds, L, cs, s, q);
  if (!stat_combine(lds, L.groups, 16 * cs, ws, tickets, R, G, NG)) return;

  const int csw = 8 * cs;
  const int c = threadIdx.x;
  const int cg = blockIdx.y * csw + c;
  if (c >= csw || cg >= C) return;
  const float sum = lds[c];
  const float sumsq = lds[csw + c];
  const float n = (float)M;
  const float mean = sum / n;
  float var = sumsq / n - mean * mean;
  if (var < 0.0f) var = 0.0f;
  mean_out[cg] = mean;
  invstd_out[cg] = rsqrtf(var + eps);
  if (update_running) {
    const float unbiased = (M > 1) ? var * n / (n - 1.0f) : var;
    running_mean[cg] += momentum * (mean - running_mean[cg]);
    running_var[cg] += momentum * (unbiased - running_var[cg]);
  }
}

// dz = dy masked by the fwd ReLU mask (if RELU); xhat = (x-mean)*invstd
template <bool RELU, int U>
__global__ __launch_bounds__(BLOCK) void bn_bwd_stats_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ dy,
    const unsigned char* __restrict__ mask, long long M, int C,
    const float* __restrict__ mean, const float* __restrict__ invstd,
    float* __restrict__ sums2, float* ws, unsigned* tickets, int G, int NG) {
  __shared__ float lds[BLOCK * 16 + 1];
  const int cpt = C >> 3;
  const int cs = min(cpt, STAT_CS);
  const int R = gridDim.x;
  const StatLane L(cs, cpt);

  F8 s1, s2;
  s1.zero();
  s2.zero();
  if (L.active) {
    const int c0 = L.c8 << 3;
    float mu[8], is[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      mu[i] = mean[c0 + i];
      is[i] = invstd[c0 + i];
    }
    const long long stride = (long long)R * L.groups;
    long long row = (long long)blockIdx.x * L.groups + L.g;
    const bf16* xp = x + c0;
    const bf16* dp = dy + c0;
    const unsigned char* mp = mask + L.c8;
    for (; row < M; row += U * stride) {  // tail: as in the fwd kernel
      short8 xr[U], dr[U];
      unsigned char mb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long r = min(row + u * stride, M - 1);
        xr[u] = *reinterpret_cast<const short8*>(xp + r * C);
        dr[u] = *reinterpret_cast<const short8*>(dp + r * C);
        mb[u] = RELU ? mp[r * cpt] : 0;
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool in = row + u * stride < M;
        const bf16* xe = reinterpret_cast<const bf16*>(&xr[u]);
        const bf16* de = reinterpret_cast<const bf16*>(&dr[u]);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float dv = bf2f(de[i]);
          const float dz = RELU ? ((mb[u] >> i) & 1 ? dv : 0.0f) : dv;
          const float xhat = (bf2f(xe[i]) - mu[i]) * is[i];
          s1.v[i] += in ? dz : 0.0f;
          s2.v[i] += in ? dz * xhat : 0.0f;
        }
      }
    }
  }
  stat_to_lds(lds, L, cs, s1, s2);
  if (!stat_combine(lds, L.groups, 16 * cs, ws, tickets, R, G, NG)) return;

  const int csw = 8 * cs;
  const int c = threadIdx.x;
  const int cg = blockIdx.y * csw + c;
  if (c >= csw || cg >= C) return;
  sums2[cg] = lds[c];
  sums2[C + cg] = lds[csw + c];
}

// ---------------------------------------------------------------------------
// fwd apply: y = [relu]( (x-mean)*invstd*gamma + beta [+ res] )
// ---------------------------------------------------------------------------

// With RELU the kernel also emits a 1-bit activation mask (one byte per
// 8-channel slot) so the backward never re-reads y — 16 B of y becomes
// 1 B of mask on the backward's critical path.
template <bool RELU, bool RES>
__global__ void bn_fwd_apply_kernel(const bf16* __restrict__ x,
                                    const bf16* __restrict__ res,
                                    bf16* __restrict__ y, long long M, int C,
                                    const float* __restrict__ mean,
                                    const float* __restrict__ invstd,
                                    const float* __restrict__ gamma,
                                    const float* __restrict__ beta,
                                    unsigned char* __restrict__ mask) {
  const int cpt = C >> 3;
  const long long total = M * cpt;
  for (long long idx = (long long)blockIdx.x * BLOCK + threadIdx.x;
       idx < total; idx += (long long)gridDim.x * BLOCK) {
    const long long row = idx / cpt;
    const int c8 = (int)(idx - row * cpt);
    const int c0 = c8 << 3;
    const long long off = row * C + c0;
    float vals[8], rv[8];
    load8(x + off, vals);
    if (RES) load8(res + off, rv);
    unsigned char mbits = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float scale = gamma[c0 + i] * invstd[c0 + i];
      float v = (vals[i] - mean[c0 + i]) * scale + beta[c0 + i];
      if (RES) v += rv[i];
      if (RELU) {
        if (v > 0.0f) mbits |= (unsigned char)(1u << i);
        else v = 0.0f;
      }
      vals[i] = v;
    }
    store8(y + off, vals);
    if (RELU) mask[idx] = mbits;
  }
}

// ---------------------------------------------------------------------------
// bwd apply: dx = gamma*invstd*(dz - s1/M - xhat*s2/M); dres = dz
// ---------------------------------------------------------------------------

template <bool RELU, bool RES>
__global__ void bn_bwd_apply_kernel(const bf16* __restrict__ x,
                                    const bf16* __restrict__ dy,
                                    const unsigned char* __restrict__ mask,
                                    bf16* __restrict__ dx,
                                    bf16* __restrict__ dres, long long M,
                                    int C, const float* __restrict__ mean,
                                    const float* __restrict__ invstd,
                                    const float* __restrict__ gamma,
                                    const float* __restrict__ sums2) {
  const int cpt = C >> 3;
  const long long total = M * cpt;
  const float rn = 1.0f / (float)M;
  for (long long idx = (long long)blockIdx.x * BLOCK + threadIdx.x;
       idx < total; idx += (long long)gridDim.x * BLOCK) {
    const long long row = idx / cpt;
    const int c8 = (int)(idx - row * cpt);
    const int c0 = c8 << 3;
    const long long off = row * C + c0;
    float xv[8], dv[8], dzv[8];
    load8(x + off, xv);
    load8(dy + off, dv);
    const unsigned char mbits = RELU ? mask[idx] : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = c0 + i;
      float dz = RELU ? ((mbits >> i) & 1 ? dv[i] : 0.0f) : dv[i];
      dzv[i] = dz;
      float xhat = (xv[i] - mean[c]) * invstd[c];
      dv[i] = gamma[c] * invstd[c] *
              (dz - sums2[c] * rn - xhat * sums2[C + c] * rn);
    }
    store8(dx + off, dv);
    if (RES) store8(dres + off, dzv);
  }
}

inline int grid_for_rows(long long M, int C) {
  int groups = max(1, BLOCK / (C >> 3));
  long long blocks = (M + groups - 1) / groups;
  return (int)(blocks < MAX_GRID ? (blocks > 0 ? blocks : 1) : MAX_GRID);
}

inline int grid_for_elems(long long elems) {
  long long blocks = (elems + BLOCK - 1) / BLOCK;
  return (int)(blocks < MAX_GRID ? (blocks > 0 ? blocks : 1) : MAX_GRID);
}

}  // namespace

#define STREAM reinterpret_cast<hipStream_t>(stream)

extern "C" {

int bps_bn_ticket_words(void) { return BN_TICKET_WORDS; }

long long bps_bn_stats_ws_floats(long long M, int C, int bwd) {
  if ((C & 7) || C < 8 || C > 2048) return -1;
  return stat_ws_floats(stat_geom(M, C, bwd ? BWD_U : FWD_U));
}

int bps_bn_fwd_stats(const void* x, long long M, int C, float eps,
                     float momentum, void* mean_out, void* invstd_out,
                     void* running_mean, void* running_var,
                     int update_running, void* ws, void* tickets,
                     void* stream) {
  if ((C & 7) || C < 8 || C > 2048) return -1;
  const StatGeom g = stat_geom(M, C, FWD_U);
  hipLaunchKernelGGL((bn_fwd_stats_kernel<FWD_U>), dim3(g.R, g.S),
                     dim3(BLOCK), 0, STREAM, (const bf16*)x, M, C, eps,
                     momentum, (float*)mean_out, (float*)invstd_out,
                     (float*)running_mean, (float*)running_var,
                     update_running, (float*)ws, (unsigned*)tickets, g.G,
                     g.NG);
  return (int)hipGetLastError();
}

int bps_bn_fwd_apply(const void* x, const void* res, void* y, long long M,
                     int C, const void* mean, const void* invstd,
                     const void* gamma, const void* beta, int relu,
                     void* mask, void* stream) {
  if ((C & 7) || C > 2048) return -1;
  if (relu && !mask) return -2;
  int g = grid_for_elems(M * (C >> 3));
#define LAUNCH_FWD(R, S)                                                    \
  hipLaunchKernelGGL((bn_fwd_apply_kernel<R, S>), dim3(g), dim3(BLOCK), 0,  \
                     STREAM, (const bf16*)x, (const bf16*)res, (bf16*)y, M, \
                     C, (const float*)mean, (const float*)invstd,           \
                     (const float*)gamma, (const float*)beta,               \
                     (unsigned char*)mask)
  if (relu && res) LAUNCH_FWD(true, true);
  else if (relu) LAUNCH_FWD(true, false);
  else if (res) LAUNCH_FWD(false, true);
  else LAUNCH_FWD(false, false);
#undef LAUNCH_FWD
  return (int)hipGetLastError();
}

int bps_bn_bwd_stats(const void* x, const void* dy, const void* mask,
                     long long M, int C, const void* mean,
                     const void* invstd, void* sums2, int relu, void* ws,
                     void* tickets, void* stream) {
  if ((C & 7) || C < 8 || C > 2048) return -1;
  if (relu && !mask) return -2;
  const StatGeom g = stat_geom(M, C, BWD_U);
#define LAUNCH_BWD_STATS(RL)                                                 \
  hipLaunchKernelGGL((bn_bwd_stats_kernel<RL, BWD_U>), dim3(g.R, g.S),        \
                     dim3(BLOCK), 0, STREAM, (const bf16*)x,                 \
                     (const bf16*)dy, (const unsigned char*)mask, M, C,      \
                     (const float*)mean, (const float*)invstd,               \
                     (float*)sums2, (float*)ws, (unsigned*)tickets, g.G,     \
                     g.NG)
  if (relu) LAUNCH_BWD_STATS(true);
  else LAUNCH_BWD_STATS(false);
#undef LAUNCH_BWD_STATS
  return (int)hipGetLastError();
}

int bps_bn_bwd_apply(const void* x, const void* dy, const void* mask,
                     void* dx,
                     void* dres, long long M, int C, const void* mean,
                     const void* invstd, const void* gamma, const void* sums2,
                     int relu, void* stream) {
  if ((C & 7) || C > 2048) return -1;
  if (relu && !mask) return -2;
  int g = grid_for_elems(M * (C >> 3));
#define LAUNCH_BWD(R, S)                                                     \
  hipLaunchKernelGGL((bn_bwd_apply_kernel<R, S>), dim3(g), dim3(BLOCK), 0,   \
                     STREAM, (const bf16*)x, (const bf16*)dy,                \
                     (const unsigned char*)mask, (bf16*)dx, (bf16*)dres,     \
                     M, C,                                                   \
                     (const float*)mean, (const float*)invstd,               \
                     (const float*)gamma, (const float*)sums2)
  if (relu && dres) LAUNCH_BWD(true, true);
  else if (relu) LAUNCH_BWD(true, false);
  else if (dres) LAUNCH_BWD(false, true);
  else LAUNCH_BWD(false, false);
#undef LAUNCH_BWD
  return (int)hipGetLastError();
}

}  // extern "C"
