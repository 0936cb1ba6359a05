// Image preprocessing on the device: the decoded uint8 RGB images of a batch -> the network input.
//
// Replaces inception_preprocessing_radix.preprocess_image for the captioning pipeline (reference
// common/inputs/preprocessing/inception_preprocessing_radix.py:158-278 as used by
// manager_image_caption.py:111-228): uint8 -> float [0,1] -> TF-1 bilinear resize to 256x256
// (tf.image.resize_images, align_corners=False: src = dst * in/out, no half-pixel offset) -> optional horizontal
// flip -> 224x224 (or any h x w) crop at (oy, ox) -> (x - 0.5) * 2.  The host keeps JPEG decoding only.  float32
// arithmetic at TF-1.9's rounding points (convert_image_dtype: cast * (1/255); resize_bilinear_op.cc compute_lerp:
// top = tl + (tr - tl) * xl, bottom likewise, out = top + (bottom - top) * yl); contraction into FMAs is
// switched off (#pragma clang fp contract(off)) so every operation rounds on its own.  Parity reference: oracle/preprocess_ref.py (bit-identical).
// comic_image_preprocess_aug: the same launch with the training augmentations of augment_dev.h (a box of the source image
// instead of the resize and the window, slim's distort_color), which the reference carries at :45-156 and never calls.
#include "augment_dev.h"

namespace {

__device__ __forceinline__ void read_taps(const uint8_t* __restrict__ src, int in_w, const Taps& t, float (&v)[3]) {
  const uint8_t* r0 = src + (size_t)t.y0 * in_w * 3;
  const uint8_t* r1 = src + (size_t)t.y1 * in_w * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    v[c] = bilinear_u8(r0[t.x0 * 3 + c], r0[t.x1 * 3 + c], r1[t.x0 * 3 + c], r1[t.x1 * 3 + c], t.wy, t.wx);
}

__global__ __launch_bounds__(256) void image_preprocess_kernel(const uint8_t* __restrict__ blob,
                                                               const ImgDesc* __restrict__ desc, float* __restrict__ dst,
                                                               int out_h, int out_w, int resize) {
  const int i = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= out_h * out_w) return;
  const ImgDesc d = desc[i];
  float v[3];
  read_taps(blob + d.offset, d.in_w, taps_legacy(d, p / out_w, p % out_w, resize), v);
  float* o = dst + ((size_t)i * out_h * out_w + p) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = to_network_range(v[c]);
}

// The same with a comic_image_aug record beside every descriptor: the box geometry and the colour ops of augment_dev.h.
// SUMS: the first of two passes of a batch with contrast ops -- the pixel up to its contrast op, added to the image's
// channel sums (images without a contrast op leave at once); otherwise the pass that writes dst.
template <bool SUMS>
__global__ __launch_bounds__(256) void image_preprocess_aug_kernel(const uint8_t* __restrict__ blob,
                                                                   const ImgDesc* __restrict__ desc,
                                                                   const ImgAug* __restrict__ aug, long long* __restrict__ sums,
                                                                   float* __restrict__ dst, int out_h, int out_w, int resize) {
  const int i = blockIdx.y;
  const ImgAug a = aug[i];
  const int at = aug_contrast_at(a);
  if (SUMS && at == 4) return;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = p < out_h * out_w;
  if (!SUMS && !live) return;
  float v[3] = {0.f, 0.f, 0.f};
  if (live) {
    const ImgDesc d = desc[i];
    const int y = p / out_w, x = p % out_w;
    read_taps(blob + d.offset, d.in_w, a.mode == COMIC_AUG_BOX ? taps_box(d, a, y, x, out_w) : taps_legacy(d, y, x, resize), v);
  }
  if (SUMS) {
    if (live) colour_ops_until(a, at, v);
    aug_accumulate(v, live, sums + 3 * i);
  } else {
    float mean[3] = {0.f, 0.f, 0.f};
    if (at < 4) {
#pragma unroll
      for (int c = 0; c < 3; ++c) mean[c] = aug_mean(sums[3 * i + c], out_h * out_w);
    }
    colour_ops_all(a, mean, v);
    float* o = dst + ((size_t)i * out_h * out_w + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = to_network_range(v[c]);
  }
}

}  // namespace

extern "C" int comic_image_preprocess(const uint8_t* blob, const void* desc, int n, float* dst, int out_h, int out_w,
                                      int resize, void* stream) {
  COMIC_REQUIRE(blob && desc && dst, "image_preprocess: null pointer");
  COMIC_REQUIRE(n > 0 && out_h > 0 && out_w > 0 && resize >= out_h && resize >= out_w, "image_preprocess: bad sizes");
  hipLaunchKernelGGL(image_preprocess_kernel, dim3(cdiv(out_h * out_w, 256), n), dim3(256), 0, (hipStream_t)stream, blob,
                     (const ImgDesc*)desc, dst, out_h, out_w, resize);
  COMIC_LAUNCH_CHECK("image_preprocess");
  return 0;
}

extern "C" int comic_image_preprocess_aug(const uint8_t* blob, const void* desc, const void* aug, int contrast, void* aug_ws,
                                          int n, float* dst, int out_h, int out_w, int resize, void* stream) {
  COMIC_REQUIRE(blob && desc && aug && aug_ws && dst, "image_preprocess_aug: null pointer");
  COMIC_REQUIRE(n > 0 && out_h > 0 && out_w > 0 && resize >= out_h && resize >= out_w, "image_preprocess_aug: bad sizes");
  COMIC_REQUIRE(((uintptr_t)aug_ws & 7) == 0, "image_preprocess_aug: workspace alignment");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(cdiv(out_h * out_w, 256), n);
  if (contrast) {
    if (hipMemsetAsync(aug_ws, 0, (size_t)n * 3 * sizeof(long long), st) != hipSuccess) {
      comic_set_error("image_preprocess_aug: clearing the workspace failed");
      return 1;
    }
    hipLaunchKernelGGL(image_preprocess_aug_kernel<true>, grid, dim3(256), 0, st, blob, (const ImgDesc*)desc,
                       (const ImgAug*)aug, (long long*)aug_ws, dst, out_h, out_w, resize);
    COMIC_LAUNCH_CHECK("image_preprocess_aug (sums)");
  }
  hipLaunchKernelGGL(image_preprocess_aug_kernel<false>, grid, dim3(256), 0, st, blob, (const ImgDesc*)desc,
                     (const ImgAug*)aug, (long long*)aug_ws, dst, out_h, out_w, resize);
  COMIC_LAUNCH_CHECK("image_preprocess_aug");
  return 0;
}
