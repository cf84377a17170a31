// csrc/objtext_math.h compiled for the host: the text the device composes, so that it can be held to objtext.py's numpy
// restatement and to utils.write_obj without a GPU, under the sanitizers (tests/_objtext_cases.py: run_host).
//
//   objtext_host <in> <out>
// in:  int64 V, F, cap; float32 verts[V][3]; int32 faces[F][3]
// out: int64 the file's full length; the min(length, cap) bytes written into a buffer of exactly cap bytes
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "objtext_math.h"

template <class T>
static bool read_n(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int64_t h[3];
  if (!read_n(in, h, 3)) return 4;
  const int64_t V = h[0], F = h[1], cap = h[2];
  if (V < 0 || F < 0 || cap < 0) return 4;
  std::vector<float> verts((size_t)V * 3);
  std::vector<int32_t> faces((size_t)F * 3);
  if (!read_n(in, verts.data(), verts.size()) || !read_n(in, faces.data(), faces.size())) return 4;
  fclose(in);

  // exactly cap bytes from the allocator, so that a byte written at or past cap is an error the sanitizer reports
  uint8_t* text = (uint8_t*)malloc(cap ? (size_t)cap : 1);
  if (!text) return 7;
  const int64_t total = objtext_host_file(verts.data(), faces.data(), V, F, cap ? text : nullptr, cap);
  // the lengths the count kernel computes, against the bytes the emit kernel puts
  int64_t sum = 0;
  for (int64_t v = 0; v < V; ++v) {
    uint32_t w[3];
    __builtin_memcpy(w, &verts[3 * (size_t)v], sizeof(w));
    const int32_t n = objtext_vertex_len(w);
    if (n > OBJTEXT_MAX_VERTEX_LINE) return 8;
    sum += n;
  }
  for (int64_t f = 0; f < F; ++f) {
    const int32_t n = objtext_face_len(&faces[3 * (size_t)f]);
    if (n > OBJTEXT_MAX_FACE_LINE) return 8;
    sum += n;
  }
  if (sum != total) return 9;

  FILE* o = fopen(argv[2], "wb");
  if (!o) return 5;
  fwrite(&total, sizeof(total), 1, o);
  fwrite(text, 1, (size_t)(total < cap ? total : cap), o);
  free(text);
  return fclose(o) == 0 ? 0 : 6;
}
