// csrc/render_math.h compiled for the host: a sequential z-buffer over the header's own functions, so that the rules the
// device runs can be held to render.py's numpy restatement without a GPU (tests/_render_cases.py: run_host).
//
//   render_host <in> <out>
// in:  int64 V, F, H, W, mode, map_size, shade, alpha256, has_background; float32 T[12], eye[4], z_near;
//      float32 verts[V][3]; int32 faces[F][3]; uint8 background[H][W][3] when has_background
// out: int32 face_id[H][W]; float32 depth[H][W]; int32 stats[8]; uint8 rgb[H][W][3]
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "render_math.h"

template <class T>
static bool read_n(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int64_t h[9];
  float T[12], eye[4], z_near;
  if (!read_n(in, h, 9) || !read_n(in, T, 12) || !read_n(in, eye, 4) || !read_n(in, &z_near, 1)) return 4;
  const int64_t V = h[0], F = h[1];
  const int H = (int)h[2], W = (int)h[3], mode = (int)h[4], map_size = (int)h[5], shade = (int)h[6], alpha256 = (int)h[7];
  std::vector<float> verts((size_t)V * 3);
  std::vector<int32_t> faces((size_t)F * 3);
  std::vector<uint8_t> background(h[8] ? (size_t)H * W * 3 : 0);
  if (!read_n(in, verts.data(), verts.size()) || !read_n(in, faces.data(), faces.size()) ||
      !read_n(in, background.data(), background.size()))
    return 4;
  fclose(in);

  std::vector<uint64_t> keys((size_t)H * W, RENDER_BACKGROUND_KEY);
  int32_t stats[RENDER_N_STATS] = {0};
  for (int64_t f = 0; f < F; ++f) {
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) {
      ++stats[RENDER_BAD_INDEX];
      continue;
    }
    const RenderVert ra = render_vertex(T, mode, map_size, W, H, z_near, &verts[3 * (size_t)a]);
    const RenderVert rb = render_vertex(T, mode, map_size, W, H, z_near, &verts[3 * (size_t)b]);
    const RenderVert rc = render_vertex(T, mode, map_size, W, H, z_near, &verts[3 * (size_t)c]);
    RenderFace face;
    const int outcome = render_face(ra, rb, rc, W, H, face);
    ++stats[outcome];
    if (outcome != RENDER_SMALL && outcome != RENDER_LARGE) continue;
    for (int iy = face.iy0; iy <= face.iy1; ++iy)
      for (int ix = face.ix0; ix <= face.ix1; ++ix) {
        int64_t e0, e1, e2;
        if (!render_covers(face, ix, iy, e0, e1, e2)) continue;
        const uint64_t key = render_key(render_depth(face, e0, e1, e2), (int32_t)f, mode);
        uint64_t& k = keys[(size_t)iy * W + ix];
        if (key < k) k = key;
      }
  }

  std::vector<int32_t> face_id((size_t)H * W);
  std::vector<float> depth((size_t)H * W);
  std::vector<uint8_t> rgb((size_t)H * W * 3);
  for (size_t i = 0; i < keys.size(); ++i) {
    face_id[i] = render_key_face(keys[i]);
    depth[i] = render_key_depth(keys[i], mode);
    int bg[3] = {255, 255, 255}, out[3];
    if (!background.empty())
      for (int k = 0; k < 3; ++k) bg[k] = background[3 * i + k];
    for (int k = 0; k < 3; ++k) out[k] = bg[k];
    if (face_id[i] >= 0) {
      const int32_t* t = &faces[3 * (size_t)face_id[i]];
      float n[3];
      int fg[3];
      render_normal(&verts[3 * (size_t)t[0]], &verts[3 * (size_t)t[1]], &verts[3 * (size_t)t[2]], n);
      if (shade == 0) render_shade_normal(n, fg);
      else fg[0] = fg[1] = fg[2] = render_shade_lambert(n, &verts[3 * (size_t)t[0]], eye);
      for (int k = 0; k < 3; ++k) out[k] = render_blend(fg[k], bg[k], alpha256);
    }
    for (int k = 0; k < 3; ++k) rgb[3 * i + k] = (uint8_t)out[k];
  }

  FILE* o = fopen(argv[2], "wb");
  if (!o) return 5;
  fwrite(face_id.data(), sizeof(int32_t), face_id.size(), o);
  fwrite(depth.data(), sizeof(float), depth.size(), o);
  fwrite(stats, sizeof(int32_t), RENDER_N_STATS, o);
  fwrite(rgb.data(), 1, rgb.size(), o);
  return fclose(o) == 0 ? 0 : 6;
}
