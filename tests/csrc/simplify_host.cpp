// csrc/simplify_math.h compiled for the host: the per-vertex and per-cluster rules the device runs, so that they can be
// held to simplify.py's numpy restatement without a GPU (tests/_simplify_cases.py: run_host).
//
//   simplify_host <in> <out>
// in:  int64 V, K; int32 R[3]; float64 lo[3], inv[3], cell[3]; float32 verts[V][3];
//      int64 S[K][3]; int64 n[K]; int32 ci[K][3]
// out: per vertex int32 {valid, i0, i1, i2, q0, q1, q2, key} (zeros behind valid = 0); float32 points[K][3]
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "simplify_math.h"

template <class T>
static bool read_n(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int64_t h[2];
  int32_t R[3];
  double lo[3], inv[3], cell[3];
  if (!read_n(in, h, 2) || !read_n(in, R, 3) || !read_n(in, lo, 3) || !read_n(in, inv, 3) || !read_n(in, cell, 3)) return 4;
  const int64_t V = h[0], K = h[1];
  if (V < 0 || K < 0) return 4;
  std::vector<float> verts((size_t)V * 3);
  std::vector<int64_t> S((size_t)K * 3), n((size_t)K);
  std::vector<int32_t> ci((size_t)K * 3);
  if (!read_n(in, verts.data(), verts.size()) || !read_n(in, S.data(), S.size()) || !read_n(in, n.data(), n.size()) ||
      !read_n(in, ci.data(), ci.size()))
    return 4;
  fclose(in);

  std::vector<int32_t> rec((size_t)V * 8, 0);
  for (int64_t v = 0; v < V; ++v) {
    const float* p = &verts[3 * (size_t)v];
    int32_t* r = &rec[8 * (size_t)v];
    if (!simp_valid_vertex(p)) continue;
    r[0] = 1;
    for (int a = 0; a < 3; ++a) simp_axis(p[a], lo[a], inv[a], R[a], &r[1 + a], &r[4 + a]);
    const uint32_t key = simp_key(r[1], r[2], r[3], R[1], R[2]);
    r[7] = (int32_t)key;
    int32_t back[3];
    simp_key_cell(key, R[1], R[2], back);
    if (back[0] != r[1] || back[1] != r[2] || back[2] != r[3]) return 7;
  }
  std::vector<float> points((size_t)K * 3);
  for (int64_t c = 0; c < K; ++c)
    for (int a = 0; a < 3; ++a)
      points[3 * (size_t)c + a] = simp_point(S[3 * (size_t)c + a], n[(size_t)c], ci[3 * (size_t)c + a], lo[a], cell[a]);

  FILE* o = fopen(argv[2], "wb");
  if (!o) return 5;
  fwrite(rec.data(), sizeof(int32_t), rec.size(), o);
  fwrite(points.data(), sizeof(float), points.size(), o);
  return fclose(o) == 0 ? 0 : 6;
}
