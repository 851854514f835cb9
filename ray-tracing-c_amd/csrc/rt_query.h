// rt_query.h — batched closest-hit queries on a resident scene (rt_hip.h: rt_trace_rays_async): the
// GPU form of the reference's `objects.hittable.vtable->hit(ray, tmin, tmax, &rec, rng)`
// (src/hittable.c:38-423) for N caller-supplied rays.
//
// The traversal is rt_device.h's resumable preorder scan (pre_begin / pre_step) and the record its
// make_record, so visit order, shrinking t_max, the sphere's exclusive and the quad's inclusive bounds,
// the rng draw of a ConstantMedium and the Translate / RotateY fix-ups are the render's, which are the
// reference's.  pre_step divides and takes roots with the compiler's correctly rounded '/' and sqrtf
// (the full sequences that sqrt_core / div_core are the cores of), so a direction of any norm is exact:
// no [kDivLo, kDivHi] precondition on |d|^2.
//
// Two execution structures over the same per-lane code (trace_one / lane_*).  rt_trace_rays_async
// launches the plain one: a thread per ray, as many workgroups as the rays need.  The diagnostic build
// also has the persistent one (RT_QUERY_NAIVE=0), which lost the measurement on every batch
// (810 000 rays are 1.5 per resident lane, and a refill round costs more than the
// divergence it removes): rays arrive from memory and are not coherent, so a wave does not own a tile.
// The grid is the resident workgroups; the lanes of a wave that have no ray take the next indices of a
// global counter together (ballot + popcount, one atomic per wave per round, as rt_general.h takes
// pixels), every lane runs kSteps preorder entries of its own ray, and a lane whose scan ended writes
// its rt_hit and is refilled in the next round: no lane waits for the slowest ray of its wave while
// unclaimed rays remain.  The leading entries of the preorder (the top of the BVH, which every ray
// visits) are staged in LDS through pre_step's lds / n_lds; the whole of it when it fits.
//
// The per-lane functions are __host__ __device__: tests/native/query_host_check.cpp runs them and an
// emulation of the wave's refill rounds on the CPU under AddressSanitizer.
#pragma once
#include "rt_device.h"

namespace rt {
namespace qry {

// Two launch shapes.  The kernel needs 56 (kFeatBook1) / 81 (kFeatAll) VGPRs, so LDS,
// not registers, bounds the occupancy:
constexpr int kBlock = 256;              // five workgroups per CU, up to kLdsSmall bytes of preorder each:
constexpr size_t kLdsSmall = 32 * 1024;  //   160 KiB / 5, 5 waves per SIMD (<= 96 VGPRs)
constexpr int kBigBlock = 1024;          // a larger preorder: one workgroup per CU with up to the CU's whole
                                         //   LDS, 4 waves per SIMD (the largest workgroup)
template <int kThreads>
constexpr int kWavesPerSimd = kThreads == kBlock ? 5 : 4;
constexpr int kSteps = 32;  // preorder entries per lane between two refill rounds (8 / 32 / 128 measured:
                            //   scene 7 shuffled 961 / 1267 / 1110 Mrays/s, scene 1 919 / 1978 / 2809)

constexpr uint32_t kFlagFront = 1u, kFlagMedium = 2u;

struct QueryView {
  DScene S;            // pre / n_pre: the query's preorder (every scene kind has one)
  const float2 *rays;  // n x (o, d): 24 B each, read as three 8-byte words (the widest aligned access)
  float4 *hits;        // n x rt_hit: 48 B each, written as three 16-byte words
  int64_t n;
  float tmin, tmax;
  uint64_t rng_state, rng_seq;
  unsigned long long *counter;  // zeroed before the launch
  uint32_t n_lds;               // leading preorder entries staged in LDS
  int32_t steps;                // preorder entries per lane between two refill rounds (kSteps)
};

// A lane's ray and the state of its scan; k < 0: the lane holds no ray.
struct Lane {
  PreTrace T;
  f3 wo, wd;
  Pcg32 g;
  int64_t k;
};

// The rank of `lane` among the lanes of `want` (the wave's lanes that take a ray this round): lane
// takes index base + rank, where base is what the wave's one atomic returned for popcount(want) rays.
RT_D int claim_rank(uint64_t want, int lane) { return __builtin_popcountll(want & ((1ull << lane) - 1ull)); }

RT_D void lane_begin(const QueryView &V, Lane &L, int64_t k) {
  const float2 a = V.rays[3 * k], b = V.rays[3 * k + 1], c = V.rays[3 * k + 2];
  L.wo = mk(a.x, a.y, b.x);
  L.wd = mk(b.y, c.x, c.y);
  L.k = k;
  L.g.seed(V.rng_state, V.rng_seq + (uint64_t)k);  // (rt_trace_rays_async: rng_seq + n < 2^31)
  pre_begin(L.T, L.wo, L.wd, V.tmax);
}

// Up to `steps` entries of the lane's scan; true once it is past the last entry.
template <int F>
RT_D bool lane_advance(const QueryView &V, Lane &L, const float4 *lds, int steps) {
  for (int s = 0; s < steps; s++)
    if (pre_step<F>(V.S, L.T, L.wo, L.wd, V.tmin, L.g, lds, V.n_lds)) return true;
  return false;
}

RT_D uint32_t fbits(float x) { return __builtin_bit_cast(uint32_t, x); }
RT_D float bitsf(uint32_t x) { return __builtin_bit_cast(float, x); }

// The rt_hit of ray k: the winner's record with u, v always filled, or the miss record.
template <int F>
RT_D void write_hit(const QueryView &V, int64_t k, f3 wo, f3 wd, bool found, const Hit &h) {
  float4 w0 = make_float4(__builtin_inff(), 0.0f, 0.0f, 0.0f), w1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float4 w2 = make_float4(0.0f, bitsf(0xffffffffu), bitsf((uint32_t)RT_REF_NONE), bitsf(0u));
  if (found) {
    Rec r;
    make_record<F, true>(V.S, wo, wd, h, r);
    const bool medium = (F & RT_FEAT_MEDIUM) && rt_ref_kind(h.prim) == RT_KIND_MEDIUM;
    w0 = make_float4(h.t, r.p.x, r.p.y, r.p.z);
    w1 = make_float4(r.normal.x, r.normal.y, r.normal.z, r.u);
    w2 = make_float4(r.v, bitsf((uint32_t)r.material), bitsf((uint32_t)h.prim),
                     bitsf((r.front ? kFlagFront : 0u) | (medium ? kFlagMedium : 0u)));
  }
  float4 *dst = V.hits + 3 * k;
  dst[0] = w0, dst[1] = w1, dst[2] = w2;
}

template <int F>
RT_D void lane_finish(const QueryView &V, Lane &L) {
  write_hit<F>(V, L.k, L.wo, L.wd, L.T.found, L.T.h);
  L.k = -1;
}

// One ray from begin to end without the refill structure: the product kernel's thread.
template <int F>
RT_D void trace_one(const QueryView &V, int64_t k) {
  Lane L;
  lane_begin(V, L, k);
  while (!pre_step<F>(V.S, L.T, L.wo, L.wd, V.tmin, L.g)) {  // trace_pre's loop, from the query's t_max
  }
  lane_finish<F>(V, L);
}

#if defined(__HIPCC__)
// The persistent loop of one workgroup (lds: V.n_lds entries of dynamic LDS).
template <int F>
__device__ __forceinline__ void query_persistent(const QueryView &V, float4 *lds) {
  for (uint32_t q = threadIdx.x; q < 2u * V.n_lds; q += blockDim.x) lds[q] = V.S.pre[q];
  __syncthreads();
  const int lane = (int)(threadIdx.x & 63u);
  Lane L;
  L.k = -1;
  bool exhausted = false;  // wave-uniform: the counter has passed n
  for (;;) {
    const uint64_t want = exhausted ? 0ull : __ballot(L.k < 0);
    if (want) {
      const int first = __builtin_ctzll(want);
      const unsigned long long cnt = (unsigned long long)__popcll(want);
      unsigned long long base = 0ull;
      if (lane == first) base = atomicAdd(V.counter, cnt);
      base = __shfl(base, first);
      if (L.k < 0) {
        const int64_t k = (int64_t)base + claim_rank(want, lane);
        if (k < V.n) lane_begin(V, L, k);
      }
      exhausted = (int64_t)(base + cnt) >= V.n;
    }
    if (__ballot(L.k >= 0) == 0ull) break;
    if (L.k >= 0 && lane_advance<F>(V, L, lds, V.steps)) lane_finish<F>(V, L);
  }
}
#endif

// rt_query.hip: the kernels over the code above, and their launches (fb: the kFeatBook1 instantiation;
// big: the kBigBlock shape).
void launch_naive(bool fb, hipStream_t st, const QueryView &V);
const void *kernel_fn(bool fb, bool big);  // (the persistent kernel: diagnostic build only)
void launch(bool fb, bool big, unsigned grid, size_t lds_bytes, hipStream_t st, const QueryView &V);

}  // namespace qry
}  // namespace rt
