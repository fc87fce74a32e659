// builder_sanitize.cpp — the host builder (csrc/bvh_build.cpp) over the box sets a bad instance record can produce, as a stand-alone
// program for `make sanitize-builder` (g++ -fsanitize=address,undefined -fsanitize=float-cast-overflow; no GPU, no Python).
// rt_set_instances turns a void record's box into the absent box before the builder sees it; the builder is nevertheless a function
// of its own, and this program feeds it what that gate keeps out as well: infinite boxes, inverted boxes, absent boxes, NaN planes and
// NaN centroids, among finite boxes and alone, at 1, 2, 300 and 5000 boxes (the exact sweep below 13 references, the binned split
// above).  It checks what has to hold whatever the boxes are: every primitive in exactly one leaf, every link inside the arrays, every
// quantised plane a 16-bit value.  The sanitizers check the rest.
// Then build_blas + quantize_bvh2 over triangle meshes with bad vertex positions (include/rt_api.h, rt_upload_geometry): every
// coordinate class of tests/bad_vertex_cases.py at 1, 2, 13, 300, 20 000 and 40 000 triangles, on 1 and 8 threads.
#include <cmath>
#include <cstdint>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "bvh_build.h"

using namespace rt;

namespace {

constexpr float INF = std::numeric_limits<float>::infinity();
const float NANF = std::numeric_limits<float>::quiet_NaN();

uint32_t rng_state = 1;
float rnd() {   // xorshift32 -> [0, 1)
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
  return (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

Aabb finite_box(float spread) {
  Aabb b;
  for (int k = 0; k < 3; k++) { const float c = (rnd() - 0.5f) * spread, h = 0.1f + rnd(); b.lo[k] = c - h; b.hi[k] = c + h; }
  return b;
}
Aabb uniform_box(float lo, float hi) { Aabb b; for (int k = 0; k < 3; k++) { b.lo[k] = lo; b.hi[k] = hi; } return b; }

// the bad boxes of the case table (tests/instance_record_cases.py) as the builder would see them without the void gate
struct BadBox { const char* name; Aabb box; };
std::vector<BadBox> bad_boxes() {
  std::vector<BadBox> v;
  v.push_back({"(-inf, inf): an infinite translation, padded; its centroid is NaN", uniform_box(-INF, INF)});
  v.push_back({"(inf, inf)", uniform_box(INF, INF)});
  v.push_back({"inverted (3e38, -3e38): NaN entries only", uniform_box(3.0e38f, -3.0e38f)});
  v.push_back({"BOX_NONE (3e38, 3e38): an empty mesh, a void record", uniform_box(3.0e38f, 3.0e38f)});
  v.push_back({"NaN planes", uniform_box(NANF, NANF)});
  v.push_back({"far: 1e30", uniform_box(1.0e30f, 1.0e30f + 1.0e25f)});
  v.push_back({"at the limit: 1e37", uniform_box(0.99e37f, 1.01e37f)});
  v.push_back({"beyond the limit: 3.4e38", uniform_box(3.3e38f, 3.4028234e38f)});
  Aabb x = finite_box(10.f); x.lo[1] = -INF; x.hi[1] = INF;   // a NaN centroid on one axis only
  v.push_back({"infinite on y only", x});
  Aabb y = finite_box(10.f); y.lo[0] = 3.0e38f; y.hi[0] = -3.0e38f;   // NaN in row 0 only: x stays inverted
  v.push_back({"inverted on x only", y});
  return v;
}

int failures = 0;
void expect(bool ok, const char* what, const char* set, uint32_t n, int max_leaf) {
  if (ok) return;
  fprintf(stderr, "FAILED: %s (%s, %u boxes, max_leaf %d)\n", what, set, n, max_leaf);
  failures++;
}

void check_tree(const BuiltBvh& t, uint32_t n, int max_leaf, const char* set) {
  // every primitive in exactly one leaf; every interior link inside the node array
  std::vector<int> seen(n, 0);
  bool links = !t.nodes.empty(), perm = t.order.size() == n;
  std::vector<int32_t> todo;
  if (links) todo.push_back(0);
  size_t visited = 0;
  while (!todo.empty() && links) {
    const int32_t e = todo.back(); todo.pop_back();
    if (++visited > t.nodes.size()) { links = false; break; }
    const int32_t ch[2] = {t.nodes[e].child0, t.nodes[e].child1};
    for (int k = 0; k < 2; k++) {
      if (ch[k] >= 0) { if ((size_t)ch[k] >= t.nodes.size()) links = false; else todo.push_back(ch[k]); continue; }
      const uint32_t ref = (uint32_t)~ch[k];
      if (e == 0 && k == 1 && t.topo[0].left < 0) continue;   // (the absent child of the synthetic root over a single leaf)
      if (max_leaf == 1) { if (ref >= n) links = false; else seen[ref]++; }
      else {
        const uint32_t first = ref >> 3, cnt = (ref & 7u) + 1u;
        if (first + cnt > n) links = false; else for (uint32_t i = first; i < first + cnt; i++) seen[t.order[i]]++;
      }
    }
  }
  expect(links, "a link leaves the arrays", set, n, max_leaf);
  for (uint32_t i = 0; i < n && perm; i++) if (t.order[i] >= n) perm = false;
  expect(perm, "order is not a permutation", set, n, max_leaf);
  bool once = true;
  for (uint32_t i = 0; i < n; i++) if (seen[i] != 1) once = false;
  expect(once || !links, "a primitive is in no leaf or in two", set, n, max_leaf);
}

void run(const std::vector<Aabb>& boxes, const std::vector<Aabb>& refit_to, const char* set) {
  const uint32_t n = (uint32_t)boxes.size();
  for (int max_leaf : {1, 4}) {
    BuiltBvh t;
    build_bvh(boxes.data(), n, max_leaf, 20, t);
    check_tree(t, n, max_leaf, set);
    Bvh4 t4;
    collapse_bvh4(t, max_leaf != 1, max_leaf == 1, t4);
    expect(!t4.nodes.empty(), "no BVH4 root", set, n, max_leaf);
    for (int pass = 0; pass < 2; pass++) {
      std::vector<BvhNodeQ> q;
      float q_lo[3], q_scale[3];
      quantize_bvh2(t, q, q_lo, q_scale);
      expect(q.size() == t.nodes.size(), "quantised node count", set, n, max_leaf);
      for (int k = 0; k < 3; k++) expect(q_scale[k] > 0.f, "q_scale is not positive", set, n, max_leaf);
      expect(bvh2_levels(q.data(), q.size(), 0) >= 1, "the quantised links are no tree", set, n, max_leaf);
      std::vector<WideNodeQ> w(q.size());
      widen_bvh2(q.data(), q.size(), 0, w.data());
      // one dequantisation shared by two trees, as a frame batch does
      double lo[3] = {3e38, 3e38, 3e38}, hi[3] = {-3e38, -3e38, -3e38};
      bvh2_bounds(t, lo, hi); bvh2_bounds(t, lo, hi);
      quant_params(lo, hi, q_lo, q_scale);
      quantize_bvh2_in(t, q, q_lo, q_scale);
      if (pass == 0 && max_leaf == 1) {   // the TLAS update: the same topology over the other box set
        refit_bvh(refit_to.data(), t);
        refit_bvh4(t, t4);
        check_tree(t, n, max_leaf, set);
      }
    }
  }
}

// ---- triangle meshes with bad vertex positions (include/rt_api.h, rt_upload_geometry; tests/bad_vertex_cases.py): build_blas + quantize_bvh2
struct CoordClass { const char* name; float value; bool whole_vertex; bool plus_minus; };
const CoordClass coord_classes[] = {
    {"NaN in y", NANF, false, false}, {"a NaN vertex", NANF, true, false}, {"+inf in y", INF, false, false}, {"-inf in y", -INF, false, false},
    {"a +inf vertex", INF, true, false}, {"a -inf vertex", -INF, true, false}, {"+inf and -inf in one triangle", INF, false, true},
    {"3e38 in y", 3.0e38f, false, false}, {"1e37 in y", 1.0e37f, false, false}, {"just below 1e37 in y", 9.9999993e36f, false, false},
    {"1e30 in y", 1.0e30f, false, false}};

int meshes = 0;
void run_mesh(uint32_t n_tris, const CoordClass& cc, int pattern, int threads) {
  // n_tris random triangles over 2 n_tris vertices (shared vertices: one bad vertex makes a fan of triangles bad)
  const uint32_t nv = 2 * n_tris + 1;
  std::vector<float> v(6ull * nv, 0.f);
  for (uint32_t i = 0; i < nv; i++) for (int k = 0; k < 3; k++) v[6ull * i + k] = (rnd() - 0.5f) * 20.f;
  std::vector<uint32_t> idx(3ull * n_tris);
  for (uint32_t t = 0; t < n_tris; t++) {
    const float c = rnd() * (float)(nv - 3);
    for (int k = 0; k < 3; k++) idx[3ull * t + k] = (uint32_t)c + (uint32_t)k;
  }
  auto chosen = [&](uint32_t i) { return pattern == 0 ? i == idx[0] : pattern == 1 ? i % 40 == 17 % std::min(40u, nv) : pattern == 2 ? i < nv / 3 + 1 : true; };
  for (uint32_t i = 0; i < nv; i++) {
    if (!chosen(i)) continue;
    if (cc.whole_vertex) for (int k = 0; k < 3; k++) v[6ull * i + k] = cc.value; else v[6ull * i + 1] = cc.value;
  }
  if (cc.plus_minus) for (uint32_t t = 0; t < n_tris; t++) if (chosen(idx[3ull * t])) v[6ull * idx[3ull * t + 1] + 1] = -INF;
  char th[8]; snprintf(th, sizeof(th), "%d", threads);
  setenv("RT_BUILD_THREADS", th, 1);
  BuiltBvh t; std::vector<TriPacket> tris;
  build_blas(v.data(), idx.data(), n_tris, t, tris);
  check_tree(t, n_tris, 4, cc.name);
  expect(tris.size() == n_tris, "packet count", cc.name, n_tris, 4);
  // the bounds hold no coordinate of a bad triangle: finite and below the limit, or empty
  bool fin = true;
  for (int k = 0; k < 3; k++) fin = fin && ((t.bounds.lo[k] > t.bounds.hi[k]) || (std::fabs(t.bounds.lo[k]) < 1e37f && std::fabs(t.bounds.hi[k]) < 1e37f));
  expect(fin, "the mesh bounds hold a bad coordinate", cc.name, n_tris, 4);
  std::vector<BvhNodeQ> q; float q_lo[3], q_scale[3];
  quantize_bvh2(t, q, q_lo, q_scale, true);
  for (int k = 0; k < 3; k++) expect(std::isfinite(q_lo[k]) && std::isfinite(q_scale[k]) && q_scale[k] > 0.f && std::isfinite(q_lo[k] + 65535.f * q_scale[k]), "the frame is not finite", cc.name, n_tris, 4);
  expect(q.size() == t.nodes.size() && bvh2_levels(q.data(), q.size(), 0) >= 1, "the quantised links are no tree", cc.name, n_tris, 4);
  Bvh4 t4; collapse_bvh4(t, true, false, t4);
  expect(!t4.nodes.empty(), "no BVH4 root", cc.name, n_tris, 4);
  meshes++;
}

}  // namespace

int main() {
  const std::vector<BadBox> bad = bad_boxes();
  int sets = 0;
  for (uint32_t n : {1u, 2u, 300u, 5000u}) {
    std::vector<Aabb> good(n);
    for (Aabb& b : good) b = finite_box(n > 300 ? 400.f : 40.f);
    for (const BadBox& bb : bad) {
      // one bad box among finite ones (in the middle), then every second box bad, then nothing but bad boxes; each set is built,
      // then refitted to the good boxes, and the good set is refitted to it (a record that turns bad in an update)
      std::vector<Aabb> one = good, half = good, all(n, bb.box);
      one[n / 2] = bb.box;
      for (uint32_t i = 0; i < n; i += 2) half[i] = bb.box;
      run(one, good, bb.name); run(half, good, bb.name); run(all, good, bb.name);
      run(good, one, bb.name); run(good, all, bb.name);
      sets += 5;
    }
    // every kind at once
    std::vector<Aabb> mixed = good;
    for (uint32_t i = 0; i < n; i++) if (i % 3 == 0) mixed[i] = bad[(i / 3) % bad.size()].box;
    run(mixed, good, "mixed"); run(good, mixed, "mixed");
    sets += 2;
  }
  printf("builder_sanitize: %d box sets, %d failures\n", sets, failures);
  // 40 000 triangles reach the threaded passes of the builder (two times Builder::PAR_MIN references); there the two patterns that
  // leave work for them
  for (uint32_t n : {1u, 2u, 13u, 300u, 20000u, 40000u})
    for (const CoordClass& cc : coord_classes)
      for (int pattern = 0; pattern < 4; pattern++)
        for (int threads : {1, 8}) {
          if (n == 40000u && pattern != 1 && pattern != 2) continue;
          run_mesh(n, cc, pattern, threads);
        }
  printf("builder_sanitize: %d triangle meshes, %d failures\n", meshes, failures);
  return failures ? 1 : 0;
}
