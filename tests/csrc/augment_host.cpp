// Host run of csrc/augment_math.h (built and run by tests/test_augment_cpu.py and tests/test_augment_gpu.py):
//   augment_host hue <shift> <out> [<in>]      augment_hue at shift 0 ... 255
//   augment_host saturation <f> <out> [<in>]   augment_saturation at the float32 nearest <f>
//   augment_host brightness <f> <out> [<in>]   augment_brightness likewise
// <in> holds RGB bytes; without it the input is every colour, pixel i = (i >> 16, (i >> 8) & 255, i & 255) for
// i < 2^24.  <out> receives the RGB bytes of the result.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "augment_math.h"

int main(int argc, char** argv) {
  if (argc != 4 && argc != 5) {
    fprintf(stderr, "usage: %s hue|saturation|brightness <value> <out> [<in>]\n", argv[0]);
    return 2;
  }
  const int op = !strcmp(argv[1], "hue") ? 0 : !strcmp(argv[1], "saturation") ? 1 : !strcmp(argv[1], "brightness") ? 2 : -1;
  if (op < 0) {
    fprintf(stderr, "unknown step %s\n", argv[1]);
    return 2;
  }
  const float f = strtof(argv[2], nullptr);
  const int shift = atoi(argv[2]);
  std::vector<uint8_t> px;
  if (argc == 5) {
    FILE* in = fopen(argv[4], "rb");
    if (!in) return perror(argv[4]), 1;
    uint8_t buf[3 << 12];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), in)) > 0;) px.insert(px.end(), buf, buf + n);
    fclose(in);
    if (px.size() % 3) return fprintf(stderr, "%s: %zu bytes are no RGB triples\n", argv[4], px.size()), 1;
  } else {
    px.resize((size_t)3 << 24);
    for (uint32_t i = 0; i < 1u << 24; ++i) px[3 * i] = i >> 16, px[3 * i + 1] = (i >> 8) & 255, px[3 * i + 2] = i & 255;
  }
  for (size_t i = 0; i < px.size(); i += 3) {
    int r = px[i], g = px[i + 1], b = px[i + 2];
    if (op == 0) augment_hue(r, g, b, shift & 255);
    else if (op == 1) augment_saturation(r, g, b, f);
    else augment_brightness(r, g, b, f);
    px[i] = (uint8_t)r, px[i + 1] = (uint8_t)g, px[i + 2] = (uint8_t)b;
  }
  FILE* out = fopen(argv[3], "wb");
  if (!out) return perror(argv[3]), 1;
  const bool ok = fwrite(px.data(), 1, px.size(), out) == px.size();
  return fclose(out) == 0 && ok ? 0 : 1;
}
