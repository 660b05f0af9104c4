// Test-time augmentation, image side: one pass's input image in one kernel (reference ultralytics/utils/torch_utils.py:270-279
// scale_img behind `x.flip(fi)` of DetectionModel._predict_augment, ultralytics/nn/tasks.py:303-318).
//
// The reference flips the image (one copy), F.interpolate()s it to (hs, ws) (a second), and F.pad()s that with 0.447 on the right
// and the bottom up to the stride multiple (Hp, Wp) (a third).  Here a lane owns four consecutive output pixels of one row: pixels
// inside (hs, ws) are the bilinear taps of dy_bilinear.h read from the source with the flip folded into the tap indices, the others
// are the pad value, and the four leave as one 16-byte store.  A pass that keeps the size (ratio 1.0 with a flip) copies the mirrored
// pixel itself.  No atomics: two runs give the same bytes.
#include "dy_host.h"
#include "../../include/dedark_yolo.h"
#include "dy_bilinear.h"

namespace {

constexpr int NT = 256;
constexpr float PAD_VALUE = 0.447f;      // torch_utils.py:279 (the ImageNet mean)

struct Si {
  const float* x; float* out;
  int planes, H, W, hs, ws, Hp, Wp, flip, same;
  float sch, scw;
};

// one thread per four consecutive output pixels of one row
__global__ __launch_bounds__(NT) void tta_scale_img_kernel(Si s) {
  const int gw = (s.Wp + 3) / 4;
  const long i = blockIdx.x * (long)NT + threadIdx.x;
  if (i >= (long)s.planes * s.Hp * gw) return;
  const int gx = (int)(i % gw);
  const long t = i / gw;
  const int y = (int)(t % s.Hp);
  const long k = t / s.Hp;
  const int xs = gx * 4, n = s.Wp - xs < 4 ? s.Wp - xs : 4;
  float v[4] = {PAD_VALUE, PAD_VALUE, PAD_VALUE, PAD_VALUE};
  if (y < s.hs && xs < s.ws) {
    const float* p = s.x + k * s.H * s.W;
    Tap ty;
    if (s.same) { ty.i0 = ty.i1 = y; ty.w1 = 0.f; }
    else ty = tap_of(y, s.sch, s.H);
    if (s.flip == 2) { ty.i0 = s.H - 1 - ty.i0; ty.i1 = s.H - 1 - ty.i1; }
    const float* ra = p + (long)ty.i0 * s.W;
    const float* rb = p + (long)ty.i1 * s.W;
    for (int e = 0; e < n; ++e) {
      const int x = xs + e;
      if (x >= s.ws) break;
      if (s.same) {
        v[e] = ra[s.flip == 3 ? s.W - 1 - x : x];
        continue;
      }
      Tap tx = tap_of(x, s.scw, s.W);
      if (s.flip == 3) { tx.i0 = s.W - 1 - tx.i0; tx.i1 = s.W - 1 - tx.i1; }
      v[e] = bilerp(ra[tx.i0], ra[tx.i1], rb[tx.i0], rb[tx.i1], tx.w1, ty.w1);
    }
  }
  const long base = (k * s.Hp + y) * s.Wp + xs;
  float* o = s.out + base;
  if (n == 4 && (base & 3) == 0) { const f32x4 q = {v[0], v[1], v[2], v[3]}; *reinterpret_cast<f32x4*>(o) = q; }
  else for (int e = 0; e < n; ++e) o[e] = v[e];
}

}  // namespace

extern "C" int dy_tta_scale_img(const float* x, int B, int C, int H, int W, int hs, int ws, int Hp, int Wp, int flip, float* out,
                                void* stream) {
  DY_CHECK(B > 0 && C > 0 && H > 0 && W > 0, "dy_tta_scale_img: empty image");
  DY_CHECK(hs > 0 && ws > 0 && Hp >= hs && Wp >= ws, "dy_tta_scale_img: resized %d x %d does not fit the padded %d x %d", hs, ws, Hp, Wp);
  DY_CHECK(flip == 0 || flip == 2 || flip == 3, "dy_tta_scale_img: flip %d (0 none, 2 up-down, 3 left-right)", flip);
  DY_CHECK(x && out && x != out, "dy_tta_scale_img: null pointer or in-place call");
  DY_CHECK(((uintptr_t)out) % 16 == 0, "dy_tta_scale_img: out must be 16-byte aligned");
  DY_CHECK((long)B * C <= INT32_MAX, "dy_tta_scale_img: too many planes");
  Si s;
  s.x = x; s.out = out; s.planes = B * C; s.H = H; s.W = W; s.hs = hs; s.ws = ws; s.Hp = Hp; s.Wp = Wp; s.flip = flip;
  s.same = hs == H && ws == W;
  s.sch = (float)H / (float)hs; s.scw = (float)W / (float)ws;
  const long groups = (long)s.planes * Hp * ((Wp + 3) / 4);
  DY_CHECK((groups + NT - 1) / NT <= INT32_MAX, "dy_tta_scale_img: too many pixels for one launch");
  dy_note_kernel("tta_scale_img_kernel");
  tta_scale_img_kernel<<<dy_cdiv(groups, NT), NT, 0, (hipStream_t)stream>>>(s);
  DY_LAUNCH_CHECK();
  return 0;
}
