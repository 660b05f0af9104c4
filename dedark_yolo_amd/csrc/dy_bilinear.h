// Bilinear taps of ATen's upsample_bilinear2d (align_corners=False, size given), shared by the mask resizes (segmask.hip) and the
// test-time-augmentation image resize (tta.hip): scale = in / out in f32, src = scale * (dst + 0.5) - 0.5 clamped at 0, i0 = (int)src,
// i1 = min(i0 + 1, in - 1), w1 = src - i0, value wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * c + wx1 * d).  The including file is
// built with -ffp-contract=off so that the index arithmetic and the weights round as written.
#pragma once

struct Tap { int i0, i1; float w1; };

__host__ __device__ inline Tap tap_of(int dst, float scale, int in) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  int i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;
  float l = src - (float)i0;
  l = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
  Tap t;
  t.i0 = i0; t.i1 = i0 < in - 1 ? i0 + 1 : i0; t.w1 = l;
  return t;
}

__device__ inline float bilerp(float a, float b, float c, float d, float wx1, float wy1) {
  const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
  return wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * c + wx1 * d);
}
