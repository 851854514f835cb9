// query_host_check — TEST INFRASTRUCTURE.  Runs the ray-query kernel's per-lane code
// (ray-tracing-c_amd/csrc/rt_query.h: lane_begin / lane_advance / lane_finish) on the CPU, built with
// AddressSanitizer, over a file of rays, and writes the rt_hit records.  The persistent kernel's wave is
// emulated serially: a few 64-lane waves take turns, each round claiming indices of one shared counter
// for its idle lanes (claim_rank), advancing every lane kSteps entries and retiring the lanes whose scan
// ended -- the claim / refill bookkeeping of query_persistent, without a GPU.  The first <n_lds> preorder
// entries are read through a separate copy, as the kernel reads them from LDS.
// tests/test_ray_query.py compares the output with tests/native/ray_query_ref.c bit for bit.
//   query_host_check <scene> <width> <rays.bin> <hits.bin> <tmin> <tmax> <rng_state> <rng_seq> <n_lds> [naive]
#include "../../ray-tracing-c_amd/csrc/rt_query.h"
#include "../../include/rt_hip.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace rt;

template <int F>
static void run_waves(const qry::QueryView &V, const float4 *lds, bool naive) {
  if (naive) {
    for (int64_t k = 0; k < V.n; k++) qry::trace_one<F>(V, k);
    return;
  }
  constexpr int kWaves = 3;
  std::vector<qry::Lane> lanes(kWaves * 64);
  for (auto &L : lanes) L.k = -1;
  bool exhausted[kWaves] = {false, false, false}, done[kWaves] = {false, false, false};
  unsigned long long counter = 0;
  for (int live = kWaves; live > 0;) {
    for (int w = 0; w < kWaves; w++) {
      if (done[w]) continue;
      qry::Lane *L = &lanes[(size_t)w * 64];
      uint64_t want = 0;
      if (!exhausted[w])
        for (int l = 0; l < 64; l++) want |= (uint64_t)(L[l].k < 0) << l;
      if (want) {
        const unsigned long long cnt = (unsigned long long)__builtin_popcountll(want), base = counter;
        counter += cnt;  // the wave's one atomic
        for (int l = 0; l < 64; l++)
          if (L[l].k < 0) {
            const int64_t k = (int64_t)base + qry::claim_rank(want, l);
            if (k < V.n) qry::lane_begin(V, L[l], k);
          }
        exhausted[w] = (int64_t)(base + cnt) >= V.n;
      }
      bool any = false;
      for (int l = 0; l < 64; l++) any |= L[l].k >= 0;
      if (!any) {
        done[w] = true;
        live--;
        continue;
      }
      for (int l = 0; l < 64; l++)
        if (L[l].k >= 0 && qry::lane_advance<F>(V, L[l], lds, qry::kSteps)) qry::lane_finish<F>(V, L[l]);
    }
  }
}

int main(int argc, char **argv) {
  if (argc < 10) {
    fprintf(stderr, "usage: query_host_check <scene> <width> <rays.bin> <hits.bin> <tmin> <tmax> <rng_state> "
                    "<rng_seq> <n_lds> [naive]\n");
    return 2;
  }
  rt_flat_scene *s = rt_scene_preset(atoi(argv[1]), atoi(argv[2]), 1, 1);
  if (!s) {
    fprintf(stderr, "preset failed: %s\n", rt_last_error());
    return 1;
  }
  FILE *f = fopen(argv[3], "rb");
  if (!f) return fprintf(stderr, "cannot read %s\n", argv[3]), 1;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  const int64_t n = bytes / (long)sizeof(rt_ray);
  std::vector<float2> rays((size_t)n * 3);
  if (n && fread(rays.data(), sizeof(rt_ray), (size_t)n, f) != (size_t)n) return fprintf(stderr, "short read\n"), 1;
  fclose(f);
  const void *arrays[13] = {s->bvh,        s->spheres,  s->quads,     s->lists,  s->list_items,
                            s->translates, s->rotates,  s->media,     s->materials, s->textures,
                            s->images,     s->perlins,  s->image_bytes};
  qry::QueryView V;
  memset(&V, 0, sizeof V);
  V.S = make_view(*s, arrays);
  std::vector<float4> pre;
  build_preorder(*s, pre);
  V.S.pre = pre.data();
  V.S.n_pre = (int32_t)(pre.size() / 2);
  int n_lds = atoi(argv[9]);
  if (n_lds > V.S.n_pre) n_lds = V.S.n_pre;
  if (n_lds < 0) n_lds = 0;
  const std::vector<float4> lds(pre.begin(), pre.begin() + 2 * (size_t)n_lds);  // exactly n_lds entries: ASan sees a read past them
  std::vector<float4> hits((size_t)n * 3);
  V.rays = rays.data();
  V.hits = hits.data();
  V.n = n;
  V.tmin = (float)atof(argv[5]);
  V.tmax = !strcmp(argv[6], "inf") ? __builtin_inff() : strtof(argv[6], nullptr);
  V.rng_state = strtoull(argv[7], nullptr, 10);
  V.rng_seq = strtoull(argv[8], nullptr, 10);
  V.n_lds = (uint32_t)n_lds;
  const bool naive = argc > 10 && !strcmp(argv[10], "naive");
  if (naive) V.n_lds = 0;
  const bool book1 = (s->features & (RT_FEAT_QUAD | RT_FEAT_XFORM | RT_FEAT_MEDIUM)) == 0;
  if (book1) run_waves<kFeatBook1>(V, lds.data(), naive);
  else run_waves<kFeatAll>(V, lds.data(), naive);
  f = fopen(argv[4], "wb");
  if (!f) return fprintf(stderr, "cannot write %s\n", argv[4]), 1;
  fwrite(hits.data(), sizeof(rt_hit), (size_t)n, f);
  fclose(f);
  printf("%lld %d %d %s\n", (long long)n, V.S.n_pre, n_lds, book1 ? "book1" : "all");
  rt_flat_free(s);
  return 0;
}
