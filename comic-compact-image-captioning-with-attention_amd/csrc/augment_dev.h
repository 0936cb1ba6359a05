// Device side of the input preprocessing that preprocess.hip (RGB blob) and jpeg_pixels.hip (component planes) share: the
// two per-image records, the source geometry of an output pixel, the bilinear combination of its four taps and the colour
// distortion of `--cnn_input_augment_color`.
//
// The augmentations are slim's distort_color and distorted_bounding_box_crop, which the reference carries and never calls
// (common/inputs/preprocessing/inception_preprocessing_radix.py:45-156; preprocess_for_train :158-234 resizes, flips and
// crops only).  Everything is float32, one rounding per operation (contraction off); the definition is restated in numpy
// by comic_amd.inputs (host path) and tests/augment_ref.py, bit for bit.
#pragma once
#include "common.h"

namespace {

struct ImgDesc {                  // comic_image_desc
  int64_t offset;                 // byte offset of the image in the uint8 blob (H x W x 3, row-major)
  int32_t in_h, in_w;
  int32_t flip, oy, ox;
  float sy, sx;                   // float32(in_h / 256), float32(in_w / 256)
};
static_assert(sizeof(ImgDesc) == 40, "comic_image_desc layout");

struct ImgAug {                   // comic_image_aug
  int32_t mode;                   // COMIC_AUG_LEGACY / COMIC_AUG_BOX
  int32_t cy, cx, ch, cw;         // the box inside the source image
  float sy, sx;                   // float32(ch / out_h), float32(cw / out_w)
  uint8_t ops[4];                 // COMIC_AUG_OP_*, applied in order
  float brightness, saturation, hue, contrast;
};
static_assert(sizeof(ImgAug) == sizeof(comic_image_aug) && sizeof(ImgAug) == 48, "comic_image_aug layout");

// a + (b - a) * w, three roundings (resize_bilinear_op.cc compute_lerp [TF-1.9]).  HIP's __f*_rn intrinsics are plain
// operators on AMD and hipcc contracts a + b * c into an FMA by default (-ffp-contract=fast): contraction is switched
// off for these functions, the TF kernel (built without FMA) rounds after the product.
__device__ __forceinline__ float lerp_rn(float a, float b, float w) {
#pragma clang fp contract(off)
  const float d = b - a;
  const float m = d * w;
  return a + m;
}

struct Taps {
  int y0, y1, x0, x1;             // rows / columns of the source image
  float wy, wx;
};

// the resize to `resize` x `resize`, the flip and the window at (oy, ox): what the kernels did before there was a box
__device__ __forceinline__ Taps taps_legacy(const ImgDesc& d, int y, int x, int resize) {
#pragma clang fp contract(off)
  const int Y = d.oy + y;
  const int X = d.flip ? resize - 1 - (d.ox + x) : d.ox + x;
  const float ys = (float)Y * d.sy, xs = (float)X * d.sx;
  Taps t;
  t.y0 = (int)floorf(ys);
  t.x0 = (int)floorf(xs);
  t.y1 = min((int)ceilf(ys), d.in_h - 1);
  t.x1 = min((int)ceilf(xs), d.in_w - 1);
  t.wy = ys - (float)t.y0;
  t.wx = xs - (float)t.x0;
  return t;
}

// resize_bilinear of the BOX straight to the output size (TF resizes the cropped tensor: the clamp is at the box edge), then
// the flip.  floor(ys) <= ch - 1 for every size in use; the min keeps a record that breaks this inside its box.
__device__ __forceinline__ Taps taps_box(const ImgDesc& d, const ImgAug& a, int y, int x, int out_w) {
#pragma clang fp contract(off)
  const int X = d.flip ? out_w - 1 - x : x;
  const float ys = (float)y * a.sy, xs = (float)X * a.sx;
  const int y0 = min((int)floorf(ys), a.ch - 1), x0 = min((int)floorf(xs), a.cw - 1);
  const int y1 = min((int)ceilf(ys), a.ch - 1), x1 = min((int)ceilf(xs), a.cw - 1);
  Taps t;
  t.wy = ys - (float)y0;
  t.wx = xs - (float)x0;
  t.y0 = a.cy + y0;
  t.y1 = a.cy + y1;
  t.x0 = a.cx + x0;
  t.x1 = a.cx + x1;
  return t;
}

// four 8-bit taps of one channel -> the [0,1] value (convert_image_dtype: cast * (1/255), then compute_lerp)
__device__ __forceinline__ float bilinear_u8(int t00, int t01, int t10, int t11, float wy, float wx) {
#pragma clang fp contract(off)
  const float inv255 = (float)(1.0 / 255);
  const float p00 = (float)t00 * inv255, p01 = (float)t01 * inv255;
  const float p10 = (float)t10 * inv255, p11 = (float)t11 * inv255;
  const float top = lerp_rn(p00, p01, wx), bot = lerp_rn(p10, p11, wx);
  return lerp_rn(top, bot, wy);
}

// [0,1] -> [-1,1] (inception_preprocessing_radix.py:269-271)
__device__ __forceinline__ float to_network_range(float v) {
#pragma clang fp contract(off)
  const float centred = v - 0.5f;
  return centred * 2.0f;
}

// ---- colour distortion ------------------------------------------------------------------------------------------------------
// t - floor(t), and 0 where that rounds up to 1 (a tiny negative t): the result lies in [0, 1)
__device__ __forceinline__ float wrap01(float t) {
#pragma clang fp contract(off)
  const float f = t - floorf(t);
  return f >= 1.0f ? 0.0f : f;
}

// v = max, d = max - min, s = d / v (0 where v <= 0), h = 0 at d = 0, else by the channel that holds the maximum (red before
// green before blue where maxima tie): (g - b) / d, 2 + (b - r) / d, 4 + (r - g) / d, times float32(1/6), wrapped into [0, 1)
__device__ __forceinline__ void rgb_to_hsv(const float (&c)[3], float& h, float& s, float& v) {
#pragma clang fp contract(off)
  const float r = c[0], g = c[1], b = c[2];
  const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
  const float d = mx - mn;
  v = mx;
  s = mx > 0.0f ? d / mx : 0.0f;
  float hh = 0.0f;
  if (d != 0.0f) {
    if (mx == r) {
      const float num = g - b;
      hh = num / d;
    } else if (mx == g) {
      const float num = b - r;
      const float q = num / d;
      hh = 2.0f + q;
    } else {
      const float num = r - g;
      const float q = num / d;
      hh = 4.0f + q;
    }
  }
  h = wrap01(hh * (float)(1.0 / 6));
}

// channel n of (5, 3, 1) for (r, g, b): k = (n + 6 h) mod 6, v - v s clamp(min(k, 4 - k), 0, 1).  n + 6 h < 12, so the
// remainder is one exact subtraction.
__device__ __forceinline__ float hsv_channel(float n, float h6, float vs, float v) {
#pragma clang fp contract(off)
  const float t = n + h6;
  const float k = t >= 6.0f ? t - 6.0f : t;
  const float m = fminf(fmaxf(fminf(k, 4.0f - k), 0.0f), 1.0f);
  const float p = vs * m;
  return v - p;
}

__device__ __forceinline__ void hsv_to_rgb(float h, float s, float v, float (&c)[3]) {
#pragma clang fp contract(off)
  const float h6 = h * 6.0f;
  const float vs = v * s;
  c[0] = hsv_channel(5.0f, h6, vs, v);
  c[1] = hsv_channel(3.0f, h6, vs, v);
  c[2] = hsv_channel(1.0f, h6, vs, v);
}

// One op of the list on the pixel's three [0,1] values.  `mean`: the channel means of the image in the state just in
// front of the contrast op (aug_mean below).
__device__ __forceinline__ void colour_op(int op, const ImgAug& a, const float (&mean)[3], float (&c)[3]) {
#pragma clang fp contract(off)
  if (op == COMIC_AUG_OP_BRIGHTNESS) {
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = c[k] + a.brightness;
  } else if (op == COMIC_AUG_OP_SATURATION) {
    float h, s, v;
    rgb_to_hsv(c, h, s, v);
    const float sf = s * a.saturation;
    hsv_to_rgb(h, fminf(fmaxf(sf, 0.0f), 1.0f), v, c);
  } else if (op == COMIC_AUG_OP_HUE) {
    float h, s, v;
    rgb_to_hsv(c, h, s, v);
    hsv_to_rgb(wrap01(h + a.hue), s, v, c);
  } else if (op == COMIC_AUG_OP_CONTRAST) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float d = c[k] - mean[k];
      const float m = d * a.contrast;
      c[k] = m + mean[k];
    }
  }
}

__device__ __forceinline__ int aug_contrast_at(const ImgAug& a) {      // position of the contrast op in the list, 4: none
  for (int j = 0; j < 4; ++j)
    if (a.ops[j] == COMIC_AUG_OP_CONTRAST) return j;
  return 4;
}

// the ops of the list in front of position `end`
__device__ __forceinline__ void colour_ops_until(const ImgAug& a, int end, float (&c)[3]) {
  const float none[3] = {0.f, 0.f, 0.f};
  for (int j = 0; j < end; ++j) colour_op(a.ops[j], a, none, c);
}

// all of them, the clamp distort_color ends with (only where there is an op: a list of none leaves the bits alone)
__device__ __forceinline__ void colour_ops_all(const ImgAug& a, const float (&mean)[3], float (&c)[3]) {
  bool any = false;
  for (int j = 0; j < 4; ++j) {
    any |= a.ops[j] != COMIC_AUG_OP_NONE;
    colour_op(a.ops[j], a, mean, c);
  }
  if (any) {
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = fminf(fmaxf(c[k], 0.0f), 1.0f);
  }
}

// The contrast mean is a sum of integers, so it does not depend on the order in which workgroups add to it: a pixel
// contributes llrint(double(v) * 2^32) per channel, mean = float32(double(sum) / (2^32 * pixels)).
__device__ __forceinline__ long long aug_fixed(float v) { return llrint((double)v * 4294967296.0); }
__device__ __forceinline__ float aug_mean(long long sum, int n_pixels) {
  return (float)((double)sum / (4294967296.0 * (double)n_pixels));
}

// First pass of a batch with contrast ops, the tail of a 256-thread workgroup: `c` is the pixel in front of its contrast
// op (`live` false for the threads behind the image's last pixel).  LDS tree, then three 64-bit atomics per workgroup.
__device__ __forceinline__ void aug_accumulate(const float (&c)[3], bool live, long long* __restrict__ sums) {
  __shared__ long long part[3][256];
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 3; ++k) part[k][t] = live ? aug_fixed(c[k]) : 0ll;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < 3; ++k) part[k][t] += part[k][t + s];
    }
    __syncthreads();
  }
  if (t < 3) atomicAdd((unsigned long long*)sums + t, (unsigned long long)part[t][0]);
}

}  // namespace
