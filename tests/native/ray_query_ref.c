/* ray_query_ref — TEST INFRASTRUCTURE: the checker of the ray-query API (include/rt_hip.h:
 * rt_trace_rays_async).  It includes the oracle's C restatement of the reference's hit methods
 * (oracle/oracle.c, unchanged) to reach its static `hit`, `rng_seed` and `Rec`, and answers a batch of
 * rays with them: hit(S, S->root, ray, tmin, tmax, &rec, rng) with ray k's rng seeded as
 * rng_seed(rng_state, rng_seq + k).  tests/test_ray_query.py compares the library's rt_hit records with
 * these bit for bit.
 *
 * The oracle's Rec carries no primitive id, so `prim` is RT_REF_NONE in every record written here; the
 * test checks the library's prim through its material and, where no transform encloses it, through
 * query_ref_prim.  A hit in a ConstantMedium is recognised by its ISOTROPIC material (only a medium's
 * phase function has one); its normal / front / u / v are stale in the reference and written as the
 * API defines them (0 / front = 1, RT_HIT_IN_MEDIUM). */
#include "../../oracle/oracle.c"

#include "../../include/rt_hip.h"

#include <string.h>

int query_ref(const rt_flat_scene *S, const rt_ray *rays, int64_t n, const rt_query_params *prm, rt_hit *hits) {
  if (!S || !rays || !prm || !hits || n < 0) return -1;
  for (int64_t k = 0; k < n; k++) {
    Rng g;
    rng_seed(&g, prm->rng_state, prm->rng_seq + (uint64_t)k);
    const Ray r = {vl(rays[k].o), vl(rays[k].d)};
    Rec rec;
    memset(&rec, 0, sizeof rec);
    rt_hit *h = &hits[k];
    memset(h, 0, sizeof *h);
    h->prim = RT_REF_NONE;
    if (!hit(S, S->root, &r, prm->tmin, prm->tmax, &rec, &g)) {
      h->t = INFINITY;
      h->material = -1;
      continue;
    }
    h->t = rec.t;
    h->p[0] = rec.p.x, h->p[1] = rec.p.y, h->p[2] = rec.p.z;
    h->material = rec.material;
    if (S->materials[rec.material].tag == RT_MAT_ISOTROPIC) {
      h->flags = RT_HIT_FRONT_FACE | RT_HIT_IN_MEDIUM;
      continue;
    }
    h->normal[0] = rec.normal.x, h->normal[1] = rec.normal.y, h->normal[2] = rec.normal.z;
    h->u = rec.u;
    h->v = rec.w;
    h->flags = rec.front ? RT_HIT_FRONT_FACE : 0u;
  }
  return 0;
}

/* The t at which `ray` hits the SPHERE / QUAD `prim` alone within the bounds, in the world frame (valid
 * for a primitive that no transform encloses).  1: hit, *t set; 0: no hit; -1: not such a primitive. */
int query_ref_prim(const rt_flat_scene *S, int32_t prim, const rt_ray *ray, float tmin, float tmax, float *t) {
  if (!S || !ray || !t || prim == RT_REF_NONE) return -1;
  const int kind = rt_ref_kind(prim);
  const int32_t i = rt_ref_index(prim);
  if (!((kind == RT_KIND_SPHERE && i < S->n_spheres) || (kind == RT_KIND_QUAD && i < S->n_quads))) return -1;
  const Ray r = {vl(ray->o), vl(ray->d)};
  Rec rec;
  memset(&rec, 0, sizeof rec);
  if (!hit(S, prim, &r, tmin, tmax, &rec, NULL)) return 0;
  *t = rec.t;
  return 1;
}
