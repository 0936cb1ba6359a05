/*
 * comic_hip.h -- C-ABI of the MI355X (gfx950) hot path of COMIC image captioning.
 *
 * The reference (jiahuei/COMIC-Compact-Image-Captioning-with-Attention) has NO FFI:
 * its hot path is a Python operator API over the TensorFlow-1.9 runtime.  Each entry
 * point below therefore replaces the TF op call-sites of one reference function and
 * cites it (file:line relative to the reference root).  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; comic_last_error()
 *     returns a thread-local description.  No exceptions cross the boundary.
 *   - all pointers are DEVICE pointers unless the name ends in _host; the caller
 *     owns every buffer (the library never allocates, frees or retains pointers).
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous on it and
 *     safe to capture in a hipGraph (no allocation / synchronisation inside).
 *   - activations NHWC; conv weights packed [Cout][Kpad] with K = (kh, kw, cin)
 *     contiguous (see comic_pack_conv_weights); dense weights row-major [in][out]
 *     (TensorFlow layout, so checkpoints map 1:1).
 *   - dtype codes: COMIC_F32 = 0, COMIC_BF16 = 1, COMIC_F16 = 2 (IEEE half storage on the f16
 *     matrix cores; forward entry points only -- the backward ones refuse it).
 */
#ifndef COMIC_HIP_H_
#define COMIC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COMIC_F32 0
#define COMIC_BF16 1
#define COMIC_F16 2
#define COMIC_ABI_VERSION 1
#define COMIC_CONV_TILES 61
#define COMIC_WS_TILE 54     /* weight-stationary 1x1 group kernel (csrc/conv_ws.hip) */
#define COMIC_IMG_TILE 55    /* image-resident kernel for stride-1 SAME convs on small maps (csrc/conv_img.hip) */
#define COMIC_CHAIN_TILE 62  /* the grouped ops are one or two CHAINS of image-resident convs (COMIC_OP_CHAIN_LINK): one launch */

const char* comic_last_error(void);
int comic_abi_version(void);
/* number of HIP devices visible; does not create a context */
int comic_device_count(void);

/* ------------------------------------------------------------------------- */
/* CNN encoder  (common/nets/inception_v3.py:100-415, inception_utils.py:32-82) */
/* ------------------------------------------------------------------------- */

/* Repack TF HWIO conv weights [kh][kw][cin][cout] (fp32) to [cout][Kpad] in `dtype`,
 * K = kh*kw*cin, Kpad = K rounded up to 64 elements, zero padded.
 * Replaces nothing in the reference (layout prep done once at checkpoint load). */
int comic_pack_conv_weights(const float* w_hwio, void* w_packed, int kh, int kw, int cin, int cout,
                            int dtype, void* stream);

/* Fold BatchNorm(inference, no gamma, eps) into per-channel scale/shift:
 * scale = rsqrt(var+eps), shift = beta - mean*scale   (inception_utils.py:56-66). */
int comic_fold_bn(const float* beta, const float* mean, const float* var, float eps, float* scale,
                  float* shift, int c, void* stream);

/* One op of a CNN forward plan. */
typedef struct comic_cnn_op {
  int32_t kind;      /* 0 conv(implicit GEMM, MFMA)  1 stem conv (cin<=4, fp32 input)
                        2 max-pool  3 avg-pool 3x3 s1 SAME (count excludes padding)
                        4 global avg-pool KHxKW VALID -> fp32
                        5 fork: the branch lanes 1..3 start after everything issued so far
                        6 join: the main lane waits for every branch lane
                        7 avg-pool 3x3 s1 SAME of an fp32 source (count excludes padding), then the
                          folded BatchNorm of weight record `weight` and ReLU: the second half of an
                          Inception pool branch whose 1x1 projection was applied BEFORE the pool
                          (both are linear and act on different axes, so they commute; the pool then
                          runs on Cout instead of Cin channels)
                        8 (bf16 plans) streaming stem: conv 3x3 VALID 32 -> 32 (weight record `weight`), conv 3x3
                          SAME 32 -> 64 (record `weight` + 1), each + BatchNorm + ReLU, then max-pool 3x3 / 2 VALID,
                          as ONE line-buffered pass (csrc/conv_stem.hip; inception_v3.py:104-111): H, W = the source
                          map, Cin 32, Cout 64, KH = KW = 3, Ho, Wo = the pooled grid; the two intermediate maps
                          are never materialised
                        9 (bf16 plans) kind 8 with Conv2d_1a_3x3 (3x3 / 2 VALID, 3 -> 32, inception_v3.py:100-104) in
                          front, in the same pass: src = the fp32 image (H, W = the image, W % 4 == 0, Cin 3), weight
                          records `weight` (Conv2d_1a, stem layout), + 1, + 2; the 32-channel map between the stem
                          conv and Conv2d_2a is never materialised either (bit-identical to kinds 1 + 8) */
  int32_t src, dst;  /* indices into the buffer table */
  int32_t src_coff, dst_coff; /* channel offsets inside src/dst (concat without a copy) */
  int32_t H, W, Cin, Cout, KH, KW, SH, SW, PT, PL, Ho, Wo;
  int32_t weight;    /* index into the weight table (conv ops) */
  int32_t relu;
  int32_t out_f32;   /* store fp32 even when the plan dtype is bf16 */
  int32_t src_f32;   /* the source buffer holds fp32 although the plan dtype is bf16
                        (global avg-pool over the fp32 attention feature map) */
  int32_t lane;      /* 0 = caller's stream; 1..3 = internal branch streams (independent
                        Inception branches run concurrently between a fork and a join) */
  int32_t tile;      /* conv: 0 = built-in heuristic, 1..COMIC_CONV_TILES = explicit kernel variant (chosen by
                        the host-side autotuner): 1..12 im2col LDS-DMA tiles / pipeline depths; 13..25
                        patch-resident variants (stride-1 layers whose input window fits the LDS: the window
                        is loaded once per tile, only the weight k-tiles stream; 4, 8 or 12 waves per
                        workgroup); 26..47 wide two-stage im2col tiles (128x128 .. 256x256, 4 or 8 waves: less LDS
                        fill per MFMA).  Ids 48..53: patch-resident variants with
                        loader waves.  Id 54 (COMIC_WS_TILE): weight-stationary kernel for 1x1 convs / groups of 1x1 convs
                        over one source with Cin <= 288 and <= 256 output channels in total (all weights in registers,
                        persistent workgroups, activation tiles streamed once).  An ineligible layer returns an error
                        for ids 13..25 and 48..61.  Ids 56..58 (59..61: the same with the walk of a pixel tile shared by two
                        workgroups that start together on one XCD): "walk" forms of 44 / 38 / 35 for grouped launches whose
                        members share their im2col matrix (the 1x1 convs at the head of an Inception block): one workgroup per
                        pixel tile walks over the out-channel tiles of all members -- the loader waves' k-tile stream runs on
                        across the tiles (no pipeline fill after the first) and the pixel rows are re-read from the L2 the
                        workgroup has just filled.  Id 55 (COMIC_IMG_TILE): image-resident kernel for the stride-1 SAME
                        convs of Mixed_5 / Mixed_6 / Mixed_7 (whole 25x25 / 12x12 / 5x5 images in the LDS without halo,
                        weights streamed global -> VGPR in fragment order: needs comic_conv_weight::w_frag).  In a group
                        the id of the first member applies to all members.  Every variant gives identical bits. */
  int32_t group;     /* conv, bf16 plans: 0 = own launch; ops that are ADJACENT in the table and
                        share a non-zero id are mutually independent (the same-depth convs of
                        the parallel Inception branches) and comic_cnn_forward_grouped runs
                        them as one launch */
  int32_t flags;     /* bit 0 (COMIC_OP_RAW), conv: store the raw product (no BatchNorm, no ReLU);
                        the epilogue is applied by a later kind-7 op */
  int32_t min_lds;   /* conv, bf16 plans: lower bound (bytes, 0 = off) on the dynamic LDS the op's workgroups request --
                        an occupancy knob for forwards that share the GPU with other kernels (84 KiB = one conv
                        workgroup per CU).  A grouped launch takes the value of its first member. */
} comic_cnn_op;
#define COMIC_OP_RAW 1
#define COMIC_OP_POOLED_SRC 2   /* bit 1, 1x1 conv of a bf16 plan: the conv reads its source through a 3x3 / stride-2 VALID
                                   max-pool (H, W = the un-pooled source, Ho, Wo = the pooled grid); the pooled map is never
                                   materialised (slim.max_pool2d + slim.conv2d 1x1, inception_v3.py:111-114,124-199) */

#define COMIC_OP_X3 4           /* bit 2, bf16 plans at fp32-class accuracy ("bf16x3" plans): every bf16 activation buffer
                                   holds a tensor of C channels as THREE channel regions [hi | lo | hi] of its 3C physical
                                   channels -- hi = bf16(v), lo = bf16(v - hi) -- and a conv's packed filter holds
                                   [W_hi | W_hi | W_lo] per tap, so that the ordinary bf16 product over 3C input channels is
                                   hi*W_hi + lo*W_hi + hi*W_lo: the split-bf16 product of the decoder's GEMMs (~2^-16 per
                                   product, fp32 accumulation) on the unchanged conv kernels.  With the bit set a conv /
                                   stem conv stores its bf16 output as the three regions (region stride = a third of the
                                   destination buffer's channels; Cout, dst_coff count channels of ONE region) and a pool
                                   reads hi + lo and writes the three regions (Cin = channels of one region); kind 7 (3x3
                                   average + BN + ReLU of an fp32 map) stores the three regions likewise.  fp32
                                   outputs (out_f32) are stored once, as always. */
#define COMIC_OP_CHAIN_LINK 8    /* bit 3, convs of a COMIC_CHAIN_TILE group (forward-only bf16 plans): this conv's output is the
                                   input of the NEXT op of the table and travels through the LDS of the workgroup that computes
                                   both (csrc/conv_img.hip, conv_img_chain_kernel: the 1x7 / 7x1 convs of a Mixed_6b-e branch,
                                   inception_v3.py:262-345) -- its dst buffer is NOT written.  The group holds one or two chains,
                                   chain after chain; an op without the bit ends its chain and stores to its dst slice.
                                   Every conv: stride 1, SAME, 12x12 maps, Cin in {128, 160, 192}; linked convs keep the
                                   channel count, a chain's last conv has 192 output channels.  Bit-identical to the same ops
                                   run one launch each. */
#define COMIC_OP_CHAIN_KEEP 16   /* bit 4, with COMIC_OP_CHAIN_LINK (trainable plans, whose backward reads every conv's output):
                                   the conv's output is ALSO stored to its dst slice, the same bits the unfused op writes. */

typedef struct comic_conv_weight {
  const void* w;       /* packed [Cout][Kpad], plan dtype (stem conv: fp32 [K][Cout]) */
  const float* scale;  /* [Cout] */
  const float* shift;  /* [Cout] */
  const void* w_frag;  /* bf16 plans, optional (NULL: tile id 55 is not eligible): the same weights in MFMA-fragment
                          order [Cout / 16][Kpad / 32][64 lanes][8] (comic_cnn_pack_frag_weights) */
} comic_conv_weight;

/* Run a whole forward plan on `stream`.  buffers[i] has buf_channels[i] channels per
 * pixel.  Replaces nets_factory.get_network_fn(...)(images) (nets/nets_factory.py:116-159;
 * src/model_base.py:72-77) for the ops listed above. */
int comic_cnn_forward(const comic_cnn_op* ops, int n_ops, void* const* buffers,
                      const int32_t* buf_channels, const comic_conv_weight* weights, int batch,
                      int dtype, void* stream);

/* w_plan: the flat bf16 weight buffer of a plan ([Cout][Kpad] records); w_frag: same size, receives every record in
 * MFMA-fragment order (lane l of k32-step s of 16-channel tile t holds W[16 t + (l & 15)][32 s + 8 (l >> 4) .. + 8]).
 * table_dev: n_weights x {element offset, Cout, Kpad} as int64 in device memory, ascending offsets; Kpad 0 = copy the
 * record unchanged up to the next offset (the fp32 stem filter). */
int comic_cnn_pack_frag_weights(const void* w_plan, void* w_frag, const int64_t* table_dev, int n_weights,
                                int64_t total_elems, void* stream);

/* Grouped execution of the same plan (bf16 plans): every run of ops with the same non-zero
 * `group` becomes ONE launch whose workgroups are spread over all member convolutions (a
 * 12x12 or 5x5 Inception stage has too few tiles per conv to fill 256 CUs at batch 64).
 * Members are convs (kind 0) and, optionally, kind-7 pool+BN+ReLU ops (elementwise work items).
 * The per-conv argument records are built once on the host and kept in device memory:
 *   n = comic_cnn_group_args_bytes(ops, n_ops)            bytes of records the plan needs
 *   comic_cnn_build_group_args(..., host_out)             fills `n` bytes (validates the ops)
 *   <caller copies host_out to device memory: group_args_dev>
 *   comic_cnn_forward_grouped(..., group_args_dev, stream)
 * Results are bit-identical to comic_cnn_forward (same kernels body, same k order). */
long comic_cnn_group_args_bytes(const comic_cnn_op* ops, int n_ops);
int comic_cnn_build_group_args(const comic_cnn_op* ops, int n_ops, void* const* buffers,
                               const int32_t* buf_channels, const comic_conv_weight* weights,
                               int batch, void* host_out);
int comic_cnn_forward_grouped(const comic_cnn_op* ops, int n_ops, void* const* buffers,
                              const int32_t* buf_channels, const comic_conv_weight* weights,
                              int batch, int dtype, const void* group_args_dev, void* stream);

/* ---- input pipeline on the device ------------------------------------------
 * The decoded uint8 RGB images of a batch -> the network input: float [0,1], TF-1 bilinear resize to
 * `resize` x `resize` (256; tf.image.resize_images with align_corners=False), optional horizontal flip, crop of
 * out_h x out_w at (oy, ox), (x - 0.5) * 2.  Replaces inception_preprocessing_radix.preprocess_image as called by
 * manager_image_caption.py:111-228; bit-identical to the numpy restatement comic_amd.inputs.preprocess_image.
 * `blob`: the images back to back (device memory); `desc`: n records (device memory). */
typedef struct comic_image_desc {
  int64_t offset;        /* byte offset of image i in `blob` (in_h x in_w x 3 uint8, row-major) */
  int32_t in_h, in_w;
  int32_t flip, oy, ox;  /* augmentation: flip of the resized image, crop origin in the resized image */
  float sy, sx;          /* float32(in_h / resize), float32(in_w / resize) */
} comic_image_desc;
int comic_image_preprocess(const uint8_t* blob, const void* desc, int n, float* dst /* [n,out_h,out_w,3] */,
                           int out_h, int out_w, int resize, void* stream);

/* Device half of the split JPEG decoder (host half: include/comic_jpeg.h, libcomic_jpeg.so).  Replaces the pixel stage of
 * tf.image.decode_jpeg / libjpeg as the reference's tf.data map runs it per image on host cores
 * (manager_image_caption.py:163-175): dequantisation + jidctint.c "ISLOW" inverse DCT, jdsample.c fancy upsampling,
 * jdcolor.c YCbCr -> RGB, in libjpeg's integer arithmetic -- the RGB bytes are the ones PIL gives for the same file
 * (oracle/jpeg_ref.py, tests/test_jpeg_split.py).
 * `coef`: the batch's quantised coefficients (device, int16, 16-byte aligned); `infos`: n comic_jpeg_info records (device)
 * with coef_base (multiple of 8 elements; comic_jpeg_pool lays the images out back to back) and pixel_off filled, ncomp == 0 for an image to skip; `max_blocks`, `max_w`,
 * `max_h`: the largest coef_count / 64, width and height among them; `planes`: scratch of as many BYTES as `coef` has
 * elements (the component planes); `pixels`: image i as height x width x 3 uint8 at pixel_off -- the blob
 * comic_image_preprocess reads. */
int comic_jpeg_pixels(const int16_t* coef, const void* infos, int n, int max_blocks, int max_w, int max_h, uint8_t* planes,
                      uint8_t* pixels, void* stream);
/* The loader's form: inverse DCT into the component planes, then comic_image_preprocess with its four taps per output
 * pixel converted from the planes on the fly (same integer upsampling / colour arithmetic, same float32 roundings: the
 * values of comic_jpeg_pixels + comic_image_preprocess, bit for bit) -- the RGB image is never written.  `desc`: n
 * comic_image_desc records (in_h / in_w / flip / crop / scales; `offset` is used for images with ncomp == 0 only, which are
 * read as RGB bytes from `blob`: the files the loader's PIL path decoded; `blob` may be NULL when there are none);
 * max_blocks 0: no image needs the inverse DCT. */
int comic_jpeg_preprocess(const int16_t* coef, const void* infos, int n, int max_blocks, uint8_t* planes, const uint8_t* blob,
                          const void* desc, float* dst /* [n,out_h,out_w,3] */, int out_h, int out_w, int resize, void* stream);
/* The same from the PACKED form of a batch (comic_jpeg.h, comic_jpeg_pool_submit_packed: per block a descriptor and the DC value,
 * per non-zero AC coefficient a 16-bit entry -- 3-4x fewer bytes across the bus than the dense blocks): a thread expands its block
 * in LDS in front of the inverse DCT.  `packed`: the batch's blob (device, 4-byte aligned, 16-bit units); image i at
 * infos[i].pixel_off, its component planes at infos[i].coef_base of `planes` (as many bytes as the images' coef_count sum).
 * Same results as comic_jpeg_preprocess on the dense coefficients, bit for bit. */
int comic_jpeg_preprocess_packed(const uint16_t* packed, const void* infos, int n, int max_blocks, uint8_t* planes,
                                 const uint8_t* blob, const void* desc, float* dst /* [n,out_h,out_w,3] */, int out_h, int out_w,
                                 int resize, void* stream);

/* Training augmentation inside the same launches (`--cnn_input_augment_crop area`, `--cnn_input_augment_color fast|full`):
 * slim's distorted_bounding_box_crop and distort_color, which the reference carries and preprocess_for_train never calls
 * (common/inputs/preprocessing/inception_preprocessing_radix.py:45-156 beside :158-234).  One comic_image_aug record per image
 * travels BESIDE its comic_image_desc (whose offset / in_h / in_w / flip hold in both modes).
 *   geometry  COMIC_AUG_LEGACY: the resize to `resize`, flip and (oy, ox) window of the descriptor, as above.
 *             COMIC_AUG_BOX: resize_bilinear_tf1(src[cy:cy+ch, cx:cx+cw], out_h, out_w), then the flip -- for output (y, x):
 *             X = flip ? out_w-1-x : x, ys = float32(y) * sy, y0 = floor(ys), y1 = min(ceil(ys), ch-1), wy = ys - y0 (x alike
 *             with X), taps at (cy + y0|y1, cx + x0|x1): the clamp is at the box edge.  No 256 x 256 intermediate.
 *   colour    on the [0,1] value of the three channels behind the lerps, ops[0..3] in order, then clamp(v, 0, 1) where there
 *             was an op, then (v - 0.5) * 2.  float32, every operation rounded on its own:
 *             BRIGHTNESS v + brightness; SATURATION rgb -> hsv, s = clamp(s * saturation, 0, 1), hsv -> rgb; HUE rgb -> hsv,
 *             h = frac(h + hue), hsv -> rgb; CONTRAST (v - mean_c) * contrast + mean_c, mean_c the channel's mean over the
 *             image's out_h * out_w output pixels in the state in front of the contrast op.
 *             rgb -> hsv: v = max, d = max - min, s = d / v (0 where v <= 0), h = 0 at d = 0, else (g-b)/d, 2 + (b-r)/d or
 *             4 + (r-g)/d by the channel holding the maximum (red before green before blue), times float32(1/6), t - floor(t)
 *             (0 where that gives 1).  hsv -> rgb, channel n = 5, 3, 1: k = n + 6h, less 6 where >= 6;
 *             v - (v * s) * clamp(min(k, 4 - k), 0, 1).
 *   mean_c    float32(double(sum) / (2^32 * out_h * out_w)), sum the int64 total of llrint(double(v) * 2^32): integers, so the
 *             order of the additions (64-bit atomics of the workgroups) does not matter and a batch gives the same bytes twice.
 * `contrast` != 0: some record holds a contrast op -- `aug_ws` (n * 3 int64, 8-byte aligned, the caller's) is cleared on the
 * stream, a first launch forms every such image's sums (images without the op leave it at once), a second one writes dst.
 * contrast == 0: ONE preprocessing launch, as the entries above. */
enum { COMIC_AUG_LEGACY = 0, COMIC_AUG_BOX = 1 };
enum { COMIC_AUG_OP_NONE = 0, COMIC_AUG_OP_BRIGHTNESS = 1, COMIC_AUG_OP_SATURATION = 2, COMIC_AUG_OP_HUE = 3,
       COMIC_AUG_OP_CONTRAST = 4 };
typedef struct comic_image_aug {
  int32_t mode;          /* COMIC_AUG_LEGACY / COMIC_AUG_BOX */
  int32_t cy, cx, ch, cw; /* the box, inside the source image (BOX) */
  float sy, sx;          /* float32(ch / out_h), float32(cw / out_w) */
  uint8_t ops[4];        /* COMIC_AUG_OP_*; every kind at most once */
  float brightness, saturation, hue, contrast;
} comic_image_aug;       /* 48 bytes */
int comic_image_preprocess_aug(const uint8_t* blob, const void* desc, const void* aug, int contrast, void* aug_ws, int n,
                               float* dst /* [n,out_h,out_w,3] */, int out_h, int out_w, int resize, void* stream);
int comic_jpeg_preprocess_aug(const int16_t* coef, const void* infos, int n, int max_blocks, uint8_t* planes, const uint8_t* blob,
                              const void* desc, const void* aug, int contrast, void* aug_ws, float* dst /* [n,out_h,out_w,3] */,
                              int out_h, int out_w, int resize, void* stream);
int comic_jpeg_preprocess_packed_aug(const uint16_t* packed, const void* infos, int n, int max_blocks, uint8_t* planes,
                                     const uint8_t* blob, const void* desc, const void* aug, int contrast, void* aug_ws,
                                     float* dst /* [n,out_h,out_w,3] */, int out_h, int out_w, int resize, void* stream);

/* ---- cnn_finetune: backward of the plan (train.py:241-249; model_base.py:76,834-849) ------
 * The CNN variables (conv weights, BN beta) become trainable; BN stays in inference mode, so a
 * conv contributes d beta = sum(1[y>0] dy), d w (backward-weight) and d x (backward-data).
 * grad_buffers[i] mirrors buffers[i] (same shape and element type; NULL where no gradient is
 * wanted, e.g. the image).  They are ACCUMULATED into: zero them, seed the gradients of the
 * plan outputs (feature map, pooled vector), then call.  Per conv weight record `grads[w]`:
 *   w_master  fp32 packed [Cout][Kpad] (stem: [K][Cout]) -- the trainable copy
 *   dw        fp32, same layout, accumulated (atomics: summation order over pixel slices is
 *             not fixed; zero it per step)
 *   dbeta     fp32 [Cout], accumulated (atomics)
 *   w_bwd     plan-dtype scratch of Cin * roundup64(KH*KW*Cout) elements for the flipped /
 *             transposed filter of the backward-data pass (NULL for the stem conv)
 * comic_cnn_refresh_weights re-derives the plan-dtype weight copy (flat bf16 conversion of all
 * masters) and shift = beta - mean*scale after an optimiser step.
 * COMIC_OP_X3 plans ("bf16x3": the same training step at fp32-class accuracy on the bf16 matrix cores): activation buffers
 * hold the three bf16 regions, grad_buffers[i] is an fp32 buffer of the LOGICAL channels (a third of buffers[i]'s; fp32
 * activation buffers as they are), masters / dw / dbeta keep the logical layout of the bf16 plan, and w_bwd holds
 * (Cin / 3) * roundup64(KH*KW*3*Cout) bf16 -- [Wt_hi | Wt_hi | Wt_lo] per tap.  Per conv: d conv as [hi | lo | hi] regions,
 * dw += x_hi dz_hi + x_lo dz_hi + x_hi dz_lo (one launch of the bf16 backward-weight kernel, three work items per tile), backward-data as the bf16
 * conv of d conv over 3 Cout channels accumulated in fp32; pools compare / sum hi + lo.  Both passes below take them (the
 * scheduled one without the fused activation gradients); the forward's [W_hi | W_hi | W_lo] copy follows the masters with
 * comic_cnn_pack_x3_weights. */
typedef struct comic_conv_grad {
  const float* w_master;
  float* dw;
  float* dbeta;
  void* w_bwd;
  int32_t bwd_tile;   /* kernel variant of the backward-data convolution (the ids of comic_cnn_op::tile; 0 = heuristic) */
  int32_t reserved;
} comic_conv_grad;
/* Two lanes: with wgrad_stream != NULL (and != stream) and a scratch of comic_cnn_backward_scratch_bytes(..., lanes = 2)
 * bytes -- every conv's d-conv tensor side by side instead of the largest one -- the weight-gradient launch of a conv goes
 * to wgrad_stream behind its act_grad launch and runs beside the backward-data chain of the earlier layers on `stream`
 * (at batch 32 neither chain fills the chip: 7.2 -> 5.x ms per cnn_finetune step).  The call joins the lanes before it
 * returns: work issued on `stream` afterwards (all-reduce, optimiser) sees every gradient.  lanes = 1 / wgrad_stream = NULL:
 * one chain on `stream`.
 * A conv the backward cannot run (stride above 2, a misaligned slice, a source with a gradient buffer whose Cin is no
 * multiple of 16: its backward-data convolution runs on the forward kernels) is refused in front of that conv's first
 * launch: its dw, dbeta and source gradient come back as they were.  (A patch-resident bwd_tile id that refuses the
 * layer is found out by its launcher, behind the conv's activation and weight gradients.) */
int64_t comic_cnn_backward_scratch_bytes(const comic_cnn_op* ops, int n_ops, int batch, int dtype, int lanes);
int comic_cnn_backward(const comic_cnn_op* ops, int n_ops, void* const* buffers,
                       void* const* grad_buffers, const int32_t* buf_channels,
                       const comic_conv_weight* weights, const comic_conv_grad* grads, int batch,
                       int dtype, int filters_ready /* 1: w_bwd already packed, see below */,
                       void* scratch, int64_t scratch_bytes, void* stream, void* wgrad_stream);
/* The same pass with the parallel branches of the Inception blocks on TWO chain lanes (cnn_finetune at batch 32 is a chain of
 * ~300 dependent small launches).  sched: n_sched rows of four int32 (action, index, lane, alt) in issue order --
 *   0 RUN       backward of ops[index] on chain lane `lane` (0: stream0, 1: stream1); alt = 1: its input gradient
 *               accumulates into grad_buffers_alt[ops[index].src] instead of grad_buffers[...] (lane 1's contributions to a
 *               block's shared input)
 *   1 FORK      stream1 waits for everything issued on stream0 so far
 *   2 JOIN_ADD  stream0 waits for stream1; index >= 0: grad_buffers[index] += grad_buffers_alt[index], the alternate buffer is
 *               cleared (alternate buffers are zero between calls)
 * Every op (kinds 5 / 6 excepted) appears exactly once, consumers before producers inside a lane; the scratch is the
 * lanes = 2 size; weight gradients go to wgrad_stream as in comic_cnn_backward.  All lanes are joined into stream0.
 * The pass fuses the activation gradient of a conv whose output has exactly one reader (a conv on the same lane: the inner
 * convs of the Inception branches) into the epilogue of that reader's backward-data launch -- one launch less per conv on the
 * serial chain of a block's longest branch.  filters_ready carries two bits here: bit 0 as in comic_cnn_backward, bit 1
 * (COMIC_CNN_BWD_NO_ACT_FUSION) runs THIS call with the unfused chain (A/B timing, parity tests). */
#define COMIC_CNN_BWD_NO_ACT_FUSION 2
int comic_cnn_backward_sched(const comic_cnn_op* ops, int n_ops, const int32_t* sched, int n_sched, void* const* buffers,
                             void* const* grad_buffers, void* const* grad_buffers_alt, const int32_t* buf_channels,
                             const comic_conv_weight* weights, const comic_conv_grad* grads, int batch, int dtype,
                             int filters_ready, void* scratch, int64_t scratch_bytes, void* stream0, void* stream1,
                             void* wgrad_stream);
/* Packs the backward-data filters of every conv from the masters (what comic_cnn_backward does per
 * conv when filters_ready == 0).  They only change with the optimiser step, so the caller can do
 * this once per step off the critical path (e.g. on a second stream during the next forward). */
/* COMIC_OP_X3 plans: the forward filter copy of n convs from their fp32 masters in one launch -- masters[i] [cout[i]][roundup64(taps[i]
 * cin[i])] (k = tap cin + ci) -> outs[i] bf16 [cout[i]][roundup64(3 taps[i] cin[i])], per tap [bf16(w) | bf16(w) | bf16(w - bf16(w))]
 * (cin = channels of ONE activation region; padding columns zero).  After an optimiser step of cnn_finetune on a bf16x3 plan. */
int comic_cnn_pack_x3_weights(const float* const* masters, void* const* outs, const int32_t* cout, const int32_t* taps,
                              const int32_t* cin, int n, void* stream);
int comic_cnn_pack_bwd_filters(const comic_cnn_op* ops, int n_ops, const comic_conv_grad* grads,
                               int dtype, void* stream);
int comic_cnn_refresh_weights(const float* master, void* plan_copy, int64_t n, const float* beta,
                              const float* mean, const float* scale, float* shift,
                              int64_t channels, void* stream);
/* The same for a plan of any 16-bit dtype: the plan copy converted to `dtype` (COMIC_BF16 or COMIC_F16);
 * comic_cnn_refresh_weights is this call with COMIC_BF16. */
int comic_cnn_refresh_weights_dtype(const float* master, void* plan_copy, int64_t n, const float* beta,
                                    const float* mean, const float* scale, float* shift,
                                    int64_t channels, int dtype, void* stream);

/* Single conv + folded BN + ReLU (slim.conv2d under inception_arg_scope). */
int comic_conv2d_bn_relu(const comic_cnn_op* op, const void* x, int x_channels, void* y,
                         int y_channels, const comic_conv_weight* wt, int batch, int dtype,
                         void* stream);

/* ------------------------------------------------------------------------- */
/* Dense algebra for the decoder (tf MatMul call-sites: common/ops.py:200-238,   */
/* ops_rnn.py:440-447,545; model_base.py:541-543,618-621)                       */
/* ------------------------------------------------------------------------- */
/* C[M,N] = alpha * op(A) * op(B) + beta * C + bias[N]      (fp32, exact-f32 MFMA)
 *   trans_a = 0: A is [M,K] (lda);  1: A is [K,M] (lda)
 *   trans_b = 0: B is [K,N] (ldb);  1: B is [N,K] (ldb)
 * bias may be NULL. */
int comic_gemm_f32(const float* A, const float* B, float* C, const float* bias, int M, int N, int K,
                   int lda, int ldb, int ldc, int trans_a, int trans_b, float alpha, float beta,
                   void* stream);

/* Same contract on the bf16 matrix cores: each fp32 operand element is split into hi + lo bf16 and a
 * product is accumulated as hi*hi + hi*lo + lo*hi in fp32 (relative error of a product <= ~2^-15,
 * ~5x the MFMA rate of the exact path).  With a workspace, shapes with few output tiles split K over
 * workgroups (partial slabs, fixed-order combine).  The decoder executors use it for the time-batched
 * products (keys, logits, weight gradients). */
int comic_gemm_f32_split3(const float* A, const float* B, float* C, const float* bias, int M, int N,
                          int K, int lda, int ldb, int ldc, int trans_a, int trans_b, float alpha,
                          float beta, void* workspace /* may be NULL: no split-K */,
                          int64_t workspace_bytes, void* stream);

/* Several independent products of the comic_gemm_f32_split3 kind in ONE launch (csrc/gemm_group.hip): the training
 * step's products outside the time loops -- the memory / rnn-init projections (common/ops_rnn.py:440-447,
 * src/model_base.py:651-689) and, after the backward loop, every weight gradient, bias sum and attention-parameter sum of
 * tf.gradients over the dense layers (src/model_base.py:325-405; common/ops.py:200-238).  A problem is
 *   C[M][N] = (alpha * op(A) op(B) + bias) [/ keep * mask] + beta * C
 * with type 0: A [K][M], B [K][N] (a weight gradient X^T dY);  1: A [M][K], B [K][N];  2: A [M][K], B [N][K];
 * ones_a: A is all ones and M = 1 (column sums of B: a bias gradient as a product; type 0).  Split-K partials are
 * combined inside the launch in slice order (bit-reproducible).  At most 20 problems; outputs must not alias inputs of
 * other problems of the call. */
typedef struct comic_gemm_prob {
  const float* A;
  const float* B;
  float* C;
  const float* bias;   /* [N] or NULL */
  const float* mask;   /* [M][ld_mask] dropout keep mask or NULL */
  int32_t M, N, K, lda, ldb, ldc, ld_mask;
  float alpha, beta, keep;
  int32_t type, ones_a;
} comic_gemm_prob;
int64_t comic_gemm_group_workspace(const comic_gemm_prob* probs, int n);
int comic_gemm_group(const comic_gemm_prob* probs, int n, void* workspace, int64_t workspace_bytes, void* stream);
/* The same call with the kernel form chosen by the caller (A/B runs and tests; comic_gemm_group is form 0):
 *   0 = as the library chooses (3 when every operand can be loaded 16 bytes at a time, 1 otherwise);
 *   1 = four waves in lockstep, two workgroups per CU (any operand alignment);
 *   2 = loader + MFMA waves, loads four k-tiles deep, one 8-wave workgroup per CU;
 *   3 = loader + MFMA waves, loads two k-tiles deep, two 8-wave workgroups per CU.
 * Forms 2 and 3 need lda % 4 == ldb % 4 == 0, A and B 16-byte aligned and K % 4 == 0 where an operand is k-contiguous
 * (types 1, 2); a form the operands do not allow returns non-zero and enqueues nothing.  The split plan depends on the
 * problems only: every form gives the same bits.
 * comic_gemm_group_resident(form in 1..3): workgroups of that form that fit one CU together
 * (hipOccupancyMaxActiveBlocksPerMultiprocessor at the form's threads and dynamic LDS); < 0 on error. */
int comic_gemm_group_form(const comic_gemm_prob* probs, int n, void* workspace, int64_t workspace_bytes, int form,
                          void* stream);
int comic_gemm_group_resident(int form);

/* Skinny product for the decode steps: out[R][N] = x[R][Kin] W[Kin][N] + bias for 33 ... 256 rows (batch x beam), Kin a
 * multiple of 8, any N -- the [TF-1.9] dense layers inside rnn_decoder_beam_search's step (BasicLSTMCell's gate product
 * model_base.py:618-621, the query layer ops_rnn.py:440-447, the output projection model_base.py:531-594) when the
 * weight matrix dwarfs the rows: W is packed to bf16 hi / lo halves in MFMA-fragment order and read from HBM exactly
 * once for all rows through an LDS-DMA stream (csrc/lstm_stream.hip), products hi*hi + hi*lo + lo*hi as
 * comic_gemm_f32_split3.  This entry packs, streams and sums in one call (the decode executors keep the packed weights
 * across the steps of a decode).  bias may be NULL. */
int64_t comic_gemm_f32_stream_workspace(int R, int Kin, int N);
int comic_gemm_f32_stream(const float* x, const float* W, const float* bias, float* out, int R, int Kin, int N,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* Same product; a caller-provided workspace lets skinny problems (M <= 2048, no trans_a)
 * split K over extra workgroups (deterministic slab reduction). */
int comic_gemm_f32_splitk(const float* A, const float* B, float* C, const float* bias, int M, int N,
                          int K, int lda, int ldb, int ldc, int trans_a, int trans_b, float alpha,
                          float beta, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* Decoder step kernels                                                       */
/* ------------------------------------------------------------------------- */
/* out[r,:] = ids[r] >= 0 ? table[ids[r],:] : 0        (model_base.py:523-526,587-593) */
int comic_embed_fwd(const float* table, const int32_t* ids, float* out, int rows, int E, int V,
                    void* stream);
/* dtable[v,:] += sum_{r: ids[r]==v} dout[r,:]   (deterministic, no atomics) */
int comic_embed_bwd(const int32_t* ids, const float* dout, float* dtable, int rows, int E, int V,
                    void* stream);

/* y = (x / keep) * mask  (tf.nn.dropout, TF-1.9 form); mask NULL -> copy */
int comic_dropout_apply(const float* x, const float* mask, float keep, float* y, int64_t n,
                        void* stream);
/* Bernoulli(keep) 0/1 masks from a counter-based generator (stateless, seed+offset). */
int comic_dropout_mask(float* mask, int64_t n, float keep, uint64_t seed, uint64_t offset,
                       void* stream);
/* same generator, seed read from device memory at run time (hipGraph replays draw new masks) */
int comic_dropout_mask_dev(float* mask, int64_t n, float keep, const uint64_t* seed_dev,
                           uint64_t offset, void* stream);
/* The four consecutive masks of a training step (n4[i] elements with keep probability keep4[i], one buffer) in one
 * launch: the same bits as four comic_dropout_mask_dev calls with cumulative offsets. */
int comic_dropout_masks4_dev(float* mask, const int64_t* n4, const float* keep4, const uint64_t* seed_dev,
                             void* stream);
/* out[0] = sum_{t,b} rows_tb[t*B + b] * w_bt[b*T + t]: the tf.contrib.seq2seq.sequence_loss reduction
 * (model_base.py:337-347) over the per-row cross-entropies of comic_decoder_train_step. */
int comic_weighted_sum_tb(const float* rows_tb, const float* w_bt, int T, int B, float* out, void* stream);

/* BasicLSTMCell gate math (model_base.py:618-621; gate order i,j,f,o; forget_bias 1).
 *  g [B,4D] pre-activations (bias included).  Writes activated gates [B,4D] (for bwd),
 *  c_new/h_new [B,D], y = dropout(h_new) [B,D].  A row is FINISHED when lens != NULL and
 *  t >= lens[b] (TrainingHelper rule); finished rows keep their state (impute_finished,
 *  ops_rnn.py:222-228): c_state = fin ? c_prev : c_new, h_state likewise.  c_prev/h_prev
 *  NULL mean zero state.  Any output pointer may be NULL. */
int comic_lstm_gates_fwd(const float* g, const float* c_prev, const float* h_prev, float* gates_act,
                         float* c_new, float* h_new, float* y, const float* mask_out, float keep_out,
                         const int32_t* lens, int t, float* c_state, float* h_state, int B, int D,
                         void* stream);
/* Backward of the above.  dc_state/dh_state are the gradients w.r.t. the carried state
 * (in/out: on return they hold the pass-through part for finished rows plus dc_prev; the
 * caller adds dh_prev from dg * K^T); dy is the gradient w.r.t. y (may be NULL).
 * dg [B,4D] is the gradient w.r.t. the pre-activations. */
int comic_lstm_gates_bwd(const float* gates_act, const float* c_prev, const float* c_new,
                         const float* dy, const float* mask_out, float keep_out, const int32_t* lens,
                         int t, float* dc_state, float* dh_state, float* dg, int B, int D, void* stream);

/* Attention descriptor shared by fwd/bwd. */
typedef struct comic_attn_desc {
  int32_t B, M, D, H, Cv;  /* keys [B,M,D]; values [B,M,Cv]; H heads */
  int32_t method;          /* 0 add_LN (ops_rnn.py:531-565)   1 dot (ops_rnn.py:611-632) */
  int32_t prob;            /* 0 softmax   1 sigmoid-normalised (model_base.py:599-603) */
  int32_t tied;            /* values alias keys (cnn_fm_projection == 'tied') */
} comic_attn_desc;

/* Fused per-step attention: score (LN-tanh-v | dot) -> per-head softmax over M ->
 * dropout(alpha) -> context.  MultiHeadAddLN.__call__ + MultiHeadAttentionWrapperV3.call
 * (ops_rnn.py:543-563, :692-716).  alpha [B,H,M] (pre-dropout, kept for backward),
 * alpha_d [B,H,M] (post-dropout = alignment history entry), ctx [B,Cv]. */
int comic_attn_step_fwd(const comic_attn_desc* d, const float* keys, const float* values,
                        const float* q, const float* ln_g, const float* ln_b, const float* v,
                        const float* tau, const float* mask_alpha, float keep_alpha, float* alpha,
                        float* alpha_d, float* ctx, void* stream);
/* Backward: given dctx [B,Cv] and the map-loss term dmap [B,M] (added to every head's
 * d alpha_d; may be NULL) produces dq [B,D]; ACCUMULATES into dkeys [B,M,D] and dvalues
 * [B,M,Cv] (same buffer when tied) and into the per-row parameter partials
 * pgrad [B, 3*D+1] = (d v | d ln_g | d ln_b | d tau). */
int comic_attn_step_bwd(const comic_attn_desc* d, const float* keys, const float* values,
                        const float* q, const float* ln_g, const float* ln_b, const float* v,
                        const float* tau, const float* alpha, const float* mask_alpha,
                        float keep_alpha, const float* dctx, const float* dmap, float* dq,
                        float* dkeys, float* dvalues, float* pgrad, void* stream);

/* sequence_loss forward+backward over time-major logits [T,B,V] (model_base.py:337-347):
 * rows with t >= lens[b] are zeroed (impute_finished), loss_rows[t*B+b] = xent*w,
 * dlogits = (softmax - onehot) * coef[b*T+t]; ids = argmax (lowest index wins). */
int comic_xent_fwd_bwd(float* logits, const int32_t* targets_bt, const float* coef_bt,
                       const float* wmask_bt, const int32_t* lens, float* loss_rows, float* dlogits,
                       int32_t* ids_tb, int T, int B, int V, void* stream);

/* ------------------------------------------------------------------------- */
/* Decoding (ops_rnn.py:49-180; tf.contrib.seq2seq BeamSearchDecoder, gather_tree) */
/* ------------------------------------------------------------------------- */
int comic_argmax_rows(const float* x, int32_t* idx, int rows, int V, void* stream);
/* One _beam_search_step: logits [B,W,V]; in/out log_probs [B,W], finished [B,W] (int32),
 * lengths [B,W] (int64); out word/parent/scores [B,W].  Ties: lower flat index first. */
int comic_beam_step(const float* logits, float* log_probs, int32_t* finished, int64_t* lengths,
                    int32_t* word_ids, int32_t* parent_ids, float* scores, int B, int W, int V,
                    int end_id, void* stream);

/* The same step from the decoder outputs y [B*W][D]: logits = y W_o + b_o (W_o [D][V], TensorFlow layout), then as
 * comic_beam_step -- with the kernels comic_decoder_beam picks for the shape: from V = 4096 (D % 128 == 0, <= 256 rows,
 * beam <= 8) the projection, log-softmax and top-k are one streaming launch over packed hi/lo W_o fragments plus a merge and
 * the logits are never written (csrc/beam_logits.hip); up to V = 1024 a beam's logits stay in a wave's registers;
 * otherwise GEMM + comic_beam_step.  Total order (score descending, flat index ascending), _mask_probs, lengths and
 * finished flags as there. */
int64_t comic_beam_step_dense_workspace(int B, int W, int D, int V);
int comic_beam_step_dense(const float* y, const float* W_o, const float* b_o, float* log_probs, int32_t* finished,
                          int64_t* lengths, int32_t* word_ids, int32_t* parent_ids, float* scores, int B, int W, int D,
                          int V, int end_id, void* workspace, int64_t workspace_bytes, void* stream);
/* Ensemble beam step (extends rnn_decoder_beam_search, common/ops_rnn.py:49-112, to several members): comic_beam_step on
 * lp[v] = log sum_m weights[m] * softmax(logits_m[b,w,:])[v], formed as A + log sum_m weights[m] * exp(a_m - A) with a_m
 * member m's log-softmax and A its maximum over the members of weight > 0 (members in order 0, 1, ...; a member of weight 0
 * is not read).  logits [n_models][B*W][V] (device), weights [n_models] (HOST: they travel as kernel arguments),
 * 1 <= n_models <= 8, W <= 64, W <= V, W*V < 2^31.  State arrays, total order, _mask_probs and the length penalty
 * (length_penalty_weight, 0 = none) as comic_beam_step / comic_decoder_beam.  With length_penalty_weight == 0,
 * W*V >= 8192 and a vocabulary of at least 2048 words the step runs split over several workgroups per entry when
 * `workspace` holds comic_beam_step_ensemble_workspace bytes (null / smaller: one workgroup per entry, same result);
 * comic_beam_step_ensemble_path() is 1 when the LAST call of this thread ran the split form. */
int64_t comic_beam_step_ensemble_workspace(int n_models, int B, int W, int V);
int comic_beam_step_ensemble(const float* logits, const float* weights, int n_models, float* log_probs, int32_t* finished,
                             int64_t* lengths, int32_t* word_ids, int32_t* parent_ids, float* scores, int B, int W, int V,
                             int end_id, float length_penalty_weight, void* workspace, int64_t workspace_bytes,
                             void* stream);
int comic_beam_step_ensemble_path(void);
/* Constrained beam search (extends rnn_decoder_beam_search, common/ops_rnn.py:49-112): what a live beam may not emit.
 * At step t a live beam with history h[0..L-1] (L == t; the start token is not part of it) bans candidate v when
 *   v is one of suppress[0..n_suppress-1], or
 *   v == end_id and lengths[beam] < min_length, or
 *   n = no_repeat_ngram > 0, L + 1 >= n, (L + 1) % ngram_stride == 0 and some window start i with i % ngram_stride == 0,
 *   i + n - 1 <= L - 1 and h[i..i+n-2] == h[L-n+1..L-1] has h[i+n-1] == v.
 * A banned candidate's step log-probability is -inf, applied after the log-softmax; finished beams ban nothing.
 * no_repeat_ngram % ngram_stride == 0, n_suppress <= 32, ids in [0,V), end_id not suppressed. */
typedef struct comic_beam_constraints {
  int32_t min_length, no_repeat_ngram, ngram_stride, n_suppress;
  int32_t suppress[32];
} comic_beam_constraints;
/* One step of the ban bookkeeping as a raw operator (common/ops_rnn.py:49-112; csrc/beam_bans.hip), to run BEFORE step t
 * on the state step t - 1 left: prev_words / prev_parents [B*W] are step t - 1's word_ids / parent_ids (null at t == 0),
 * finished [B*W], lengths [B*W] (int64).  hist [2][B*W][max_steps] (int32) holds the beams' token histories in beam
 * order: buffer (t-1)&1 is read, row (b,w) of buffer t&1 becomes row (b, parent) of it plus the word (t tokens).
 * bits [B*W][ceil(V/32)] receives the masks: bit v of a row set = banned; all zero for a finished row and at positions
 * >= V.  Parents are clamped to [0,W) and tokens to [0,V) before they index anything.  V <= 65 536. */
int comic_beam_bans(const int32_t* prev_words, const int32_t* prev_parents, const int32_t* finished, const int64_t* lengths,
                    int32_t* hist, uint32_t* bits, int t, int B, int W, int V, int max_steps, int end_id,
                    const comic_beam_constraints* constraints, void* stream);
/* comic_beam_step_ensemble (common/ops_rnn.py:49-112) under a ban mask: bits [B*W][words], words == ceil(V/32), as
 * comic_beam_bans writes it.  Every live beam must keep at least W candidates that are not banned.  An all-zero mask gives
 * comic_beam_step_ensemble's result to the bit; workspace, split form and comic_beam_step_ensemble_path() as there. */
int comic_beam_step_constrained(const float* logits, const float* weights, int n_models, float* log_probs,
                                int32_t* finished, int64_t* lengths, int32_t* word_ids, int32_t* parent_ids, float* scores,
                                int B, int W, int V, int end_id, float length_penalty_weight, const uint32_t* bits, int words,
                                void* workspace, int64_t workspace_bytes, void* stream);
/* Diverse beam search (Vijayakumar et al. 2016, Hamming diversity; extends rnn_decoder_beam_search,
 * common/ops_rnn.py:49-112): the W slots of an entry form `groups` = G groups of Wg = W / G, group g owning the slots
 * [g*Wg, (g+1)*Wg); diversity = lambda.  total[w][v] = log_probs[w] + step[w][v] and score[w][v] (total, or with a length
 * penalty total / ((5 + len) / 6)^lpw) are the plain step's, _mask_probs for finished beams and -inf for banned
 * candidates included.  The groups are processed in order g = 0 .. G-1:
 *   count[v]   = the number of slots q < g*Wg of the entry whose word chosen at this step is v;
 *   rank[w][v] = score[w][v] - lambda * count[v] for a live beam w and v != end_id, score[w][v] otherwise (a finished
 *                beam and <EOS> are never penalised); the product is float(lambda) * float(count), subtracted once;
 *   the group selects its Wg best among its own Wg * V candidates, rank descending, then entry-wide flat index
 *   f = w*V + v ascending (all -inf / NaN: the lowest untaken flat index of the group's range);
 *   slot g*Wg + r gets word = f % V, parent = f / V (an entry-wide slot, always inside the group), scores = the rank,
 *   log_probs (the state) = the UNPENALISED total, finished and lengths as ever.
 * The initial state has the first slot of every group live with log-probability 0.  G == 1 is the plain step to the bit;
 * lambda == 0 gives G identical beams of width Wg; group 0 is always beam search of width Wg.  The penalty is per token at
 * the same position (radix tokens: not per word).
 * Limits: 1 <= groups <= W, W % groups == 0, diversity finite and >= 0, Wg <= V. */
typedef struct comic_beam_groups {
  int32_t groups;
  float diversity;
} comic_beam_groups;
/* comic_beam_step_ensemble / comic_beam_step_constrained (common/ops_rnn.py:49-112) under groups, as a raw operator.
 * bits may be NULL: no bans, and `words` is ignored; else bits [B*W][words], words == ceil(V/32).  groups must not be
 * NULL.  One workgroup per entry loops over the groups; the split form (same eligibility rule, on the entry-wide W * V)
 * is the statistics once and a chunk top-k + a merge per group: 1 + 2 G launches ordered by the stream.
 * comic_beam_step_ensemble_workspace bytes suffice; comic_beam_step_ensemble_path() reports the form. */
int comic_beam_step_diverse(const float* logits, const float* weights, int n_models, float* log_probs, int32_t* finished,
                            int64_t* lengths, int32_t* word_ids, int32_t* parent_ids, float* scores, int B, int W, int V,
                            int end_id, float length_penalty_weight, const uint32_t* bits, int words,
                            const comic_beam_groups* groups, void* workspace, int64_t workspace_bytes, void* stream);
/* Beam search with required words (Anderson et al. 2017, "Guided Open Vocabulary Image Captioning with Constrained Beam
 * Search"; the bank form of Post & Vilar 2018; extends rnn_decoder_beam_search, common/ops_rnn.py:49-112): every image
 * names up to n_words = C words (1 <= C <= 4) of stride = S tokens each (1 <= S <= 4; 1 for word tokens, the radix word
 * length for radix tokens) that its caption has to contain.  banks = C*S + 1 must divide the beam width W; Wb = W / banks,
 * and slot w of an entry belongs to bank w / Wb.  The words are a DEVICE table req, int32 [B][C][S]: row (b, q) is the S
 * tokens of required word q of image b, or all -1 for "no word here"; tokens lie in [0, V) and none equals end_id.  The
 * kernels read the table at run time, so a captured graph replays with a new table.
 *   Progress of a history h[0..L-1] (the tokens emitted so far) of entry b, with k = L mod S:
 *     met_q       row q is padding, or some i with i % S == 0 and i + S <= L has h[i..i+S-1] == req[b][q];
 *     m           = #{q : met_q};
 *     partial     k > 0 and some unmet q has h[L-k..L-1] == req[b][q][0..k-1];
 *     progress(h) = S*m + (k if partial else 0), in [0, C*S].  With S == 1: the number of required words present.
 *   Destination bank of candidate (w, v): progress(h_w ++ v) for a live parent w, w / Wb for a finished one (it stays
 *   where it is; _mask_probs makes it emit <EOS> as ever).
 *   Selection, per entry and per bank c, the banks independent of each other: among the candidates of ALL W parents and
 *   all V tokens -- total and score exactly the plain step's, _mask_probs, the ban bits and the length penalty as in
 *   comic_beam_step_constrained -- those with dest == c and a finite total (not -inf, not NaN) are eligible; bank c takes
 *   its Wb best, score descending, then entry-wide flat index w*V + v ascending, into the slots c*Wb + r in rank order:
 *   word, parent (an entry-wide slot, possibly of another bank), scores = the score, log_probs (the state) = the
 *   unpenalised total, finished and lengths as the plain step.  A slot for which no eligible candidate is left is written
 *   as a DEAD slot: parent = the slot itself, word = end_id, scores = log_probs = -inf, finished = 1, lengths = the slot's
 *   own previous length (a bank is legitimately empty for many steps; this replaces the lowest-untaken-index corner).
 *   Initial state: entry b has one live slot, the first slot of bank S * (number of padding rows of b), with
 *   log-probability 0; every other slot is finished with -inf.  An image without words starts in the top bank, which is
 *   then plain beam search of width Wb.
 *   Result: slot c*Wb is bank c's best; the caption of an image is the first slot of the highest bank whose first slot
 *   has a finite final score, and met = bank / S of that slot.  Hypotheses that finish in lower banks are returned on
 *   purpose: the fallback when the full set is unreachable within max_steps.
 *   What a step needs per live row is a table: base (int32 [B*W]) = S * m of the row, where every token without a special
 *   leads, and special (int32 [B*W][4][2] of (token, dest); token -1 = unused): per unmet word q whose first k tokens are
 *   the row's tail, the token req[b][q][k] with dest S*m + k + 1 when k + 1 < S, else S * (m + the number of unmet words
 *   this token completes).  Specials that name the same token carry the same dest (the first one decides).  The step is
 *   defined on that table alone.
 * Limits: 1 <= n_words <= 4, 1 <= stride <= 4, W % (n_words*stride + 1) == 0, V <= 65 536; no beam groups, no sampling. */
typedef struct comic_beam_required {
  int32_t n_words, stride;
} comic_beam_required;
/* One step of the required-word bookkeeping as a raw operator (csrc/beam_required.hip; common/ops_rnn.py:49-112 has no
 * counterpart), to run BEFORE step t on the state step t - 1 left.  prev_words / prev_parents [B*W]: step t - 1's word_ids
 * / parent_ids (null at t == 0); req: the device table above; hist [2][B*W][max_steps]: the token histories, advanced
 * exactly as comic_beam_bans advances them (the executor keeps ONE pair when a decode has constraints too).  Writes base
 * [B*W] and special [B*W][4][2] for every row (the step consults those of live rows only).  Parents are clamped to [0,W)
 * and tokens to [0,V) before they index anything.  (Named _table: the struct has the plain name.) */
int comic_beam_required_table(const int32_t* prev_words, const int32_t* prev_parents, const int32_t* req, int32_t* hist,
                              int32_t* base, int32_t* special, const comic_beam_required* required, int t, int B, int W,
                              int V, int max_steps, int end_id, void* stream);
/* The initial state above from the table's padding rows, as a raw operator: log_probs, finished, lengths [B*W]. */
int comic_beam_required_init(const int32_t* req, float* log_probs, int32_t* finished, int64_t* lengths, int B, int W, int V,
                             int end_id, const comic_beam_required* required, void* stream);
/* comic_beam_step_ensemble / comic_beam_step_constrained (common/ops_rnn.py:49-112) under banks, as a raw operator on the
 * table (base, special) above; 2 <= banks <= 17, W % banks == 0.  bits may be NULL: no bans, and `words` is ignored.  A
 * special whose token is outside [0,V) is unused; a dest outside [0,banks) leads nowhere.  One workgroup per entry, or,
 * where comic_beam_step_ensemble would run split and `workspace` holds comic_beam_step_required_workspace bytes, the
 * statistics once and a chunk launch + a merge per bank (1 + 2 banks launches ordered by the stream);
 * comic_beam_step_ensemble_path() reports the form. */
int64_t comic_beam_step_required_workspace(int n_models, int B, int W, int V);
int comic_beam_step_required(const float* logits, const float* weights, int n_models, float* log_probs, int32_t* finished,
                             int64_t* lengths, int32_t* word_ids, int32_t* parent_ids, float* scores, int B, int W, int V,
                             int end_id, float length_penalty_weight, const uint32_t* bits, int words, const int32_t* base,
                             const int32_t* special, int banks, void* workspace, int64_t workspace_bytes, void* stream);
/* Sampling inside the beam step (extends rnn_decoder_beam_search, common/ops_rnn.py:49-112): the W slots of an entry
 * (1 <= W <= 64) are W independent chains, each drawn from the step distribution at a temperature by the Gumbel-max rule
 * with noise from a counter-based generator -- nothing is stored.  All W slots start live with log-probability 0; a
 * slot's parent is always the slot itself, so gather_tree, the state gathers and the ban / attention histories work
 * unchanged.
 *   Generator: seed_dev (DEVICE memory, read by the kernels at run time: a captured graph replays with new values) =
 *   uint64[2] = {seed, image_base}.  For entry b, slot w, step t, candidate v, with splitmix64 of csrc/splitmix.h:
 *     k1 = splitmix64(splitmix64(seed) ^ (image_base + b))
 *     k2 = splitmix64(k1 ^ ((uint64(w) << 32) | uint64(t)))
 *     r  = splitmix64(k2 ^ uint64(v));  k = r >> 41 (23 bits);  u = (2k + 1) * 2^-24 (exact in fp32, never 0, never 1)
 *     g  = -logf(-logf(u))   with the accurate logf; g in [-2.82, 16.64]
 *   The noise depends on the image's index in the run (image_base + b), not on the batch it happens to be in.
 *   Rank: lp[v] is the step log-probability of the plain step (the ensemble mean; -inf for a banned candidate of a live
 *   slot).  A live slot ranks rank[v] = lp[v] * inv_temp + g(b, w, t, v), inv_temp = 1.0f / temperature formed once on
 *   the host in fp32 (-inf stays -inf), and takes the best rank among its own V candidates, lowest v on ties (all -inf /
 *   NaN: the lowest flat index of its row).  A finished slot sees no noise: _mask_probs makes it emit <EOS>, its length
 *   freezes, its log-probability carries over.
 *   Outputs: word_ids = v, parent_ids = w, the state log_probs = old state + lp[v], scores = the same value; finished and
 *   lengths as ever.  The state is the model's UNPERTURBED, UNTEMPERED log-probability log p(caption so far | image):
 *   with temperature != 1 it is not the log-probability under the tempered distribution.  The perturbed rank is never
 *   returned.
 * Limits: temperature finite and > 0 with a finite fp32 reciprocal; no length penalty, no beam groups. */
typedef struct comic_beam_sampling {
  float temperature;
  const uint64_t* seed_dev;
} comic_beam_sampling;
/* The generator above as a raw operator (common/ops_rnn.py:49-112 has no counterpart; test aid): k_out / g_out
 * [B*W][V] (device) receive k and g of step t for every (entry, slot, candidate).  Either output may be NULL. */
int comic_beam_sample_noise(const uint64_t* seed_dev, int B, int W, int t, int V, int32_t* k_out, float* g_out,
                            void* stream);
/* comic_beam_step_ensemble / comic_beam_step_constrained (common/ops_rnn.py:49-112) under sampling, as a raw operator:
 * step t of the rule at comic_beam_sampling.  bits may be NULL: no bans, and `words` is ignored; else bits [B*W][words],
 * words == ceil(V/32).  One workgroup per entry loops over the slots; the split form (same eligibility rule, on the
 * entry-wide W * V, when `workspace` holds comic_beam_step_sampled_workspace bytes -- more than the ensemble step's: every
 * slot's candidates carry their unperturbed totals) is the statistics, ONE chunk launch that forms every slot's best per
 * chunk and ONE merge: 3 launches whatever W is.  comic_beam_step_ensemble_path() reports the form. */
int64_t comic_beam_step_sampled_workspace(int n_models, int B, int W, int V);
int comic_beam_step_sampled(const float* logits, const float* weights, int n_models, float* log_probs, int32_t* finished,
                            int64_t* lengths, int32_t* word_ids, int32_t* parent_ids, float* scores, int B, int W, int V,
                            int end_id, const uint32_t* bits, int words, const comic_beam_sampling* sampling, int t,
                            void* workspace, int64_t workspace_bytes, void* stream);
/* Top-k and nucleus (top-p) truncation of the sampled step (extends rnn_decoder_beam_search, common/ops_rnn.py:49-112):
 * which candidates a live slot may draw from.  Applied to a live slot (b, w) at step t AFTER the ban mask of the
 * constraints (if any) has been built and BEFORE the sampled step ranks; its result is ban bits in the same mask.
 *   Inputs: lp[v] is the step log-probability of the plain step (the ensemble mean, the very code the step ranks by);
 *   a[v] = lp[v] * inv_temp in fp32, inv_temp = 1.0f / temperature formed once on the host as for comic_beam_sampling;
 *   the allowed set A is the tokens whose ban bit is clear (no constraints: all V tokens).
 *   Top-k (top_k >= 1; 0 = off): K = the top_k largest a over A, equal values resolved by lowest v.  top_k >= |A|: the
 *   stage does nothing and K = A.
 *   Top-p (0 < top_p < 1; top_p >= 1 = off): m = max_K a, e[v] = exp(a[v] - m), Z = sum_K e; tau is the largest value
 *   among a[K] such that sum_{u in K, a[u] >= tau} e[u] >= top_p * Z (a product, never a division); v in K is kept iff
 *   a[v] >= tau: all candidates tied at the boundary value are kept.  The nucleus is taken on the distribution
 *   renormalised over K: the temperature -> top-k -> top-p order.  The masses are summed exactly, as the fixed-point
 *   integers floor(e * 2^40) (csrc/beam_truncate.hip), so the mask does not depend on how the waves interleave.
 *   Mask: every token of a live row that is not kept gets its ban bit set; bits already set stay set; the best allowed
 *   candidate is always kept.  A row whose m is not finite (all banned, or a NaN) is left as it came.  A finished row is
 *   not touched: _mask_probs makes it emit <EOS> as ever.
 *   Nothing else changes: the sampled step ranks lp[v] * inv_temp + g over the survivors; word_ids, the state log_probs
 *   and scores stay the model's own UNPERTURBED, UNTEMPERED, UNTRUNCATED log p(caption so far | image) -- not the
 *   log-probability under the truncated distribution.
 * Limits: top_k >= 0; top_p > 0 and not NaN; not both stages off; V <= 65 536; sampling only (no beam search, no groups). */
typedef struct comic_beam_truncation {
  int32_t top_k;
  float top_p;
} comic_beam_truncation;
/* One step of the rule above as a raw operator (common/ops_rnn.py:49-112 has no counterpart; csrc/beam_truncate.hip).
 * logits [n_models][B*W][V] (device), weights [n_models] (HOST) as comic_beam_step_ensemble; finished [B*W];
 * bits [B*W][words], words == ceil(V/32).  has_bans != 0: bits holds the constraints' mask (comic_beam_bans) and is
 * updated in place; has_bans == 0: its incoming content is ignored and every word of every row is written (a finished
 * row, and a row left as it came, as zeros).  Bits at positions >= V stay / become zero.  As a raw operator a top_k that
 * reaches V is accepted (it changes nothing).  workspace: comic_beam_truncate_workspace bytes (0 while a row's keys fit
 * in LDS, V <= 32 768; else a scratch row per slot), may be NULL when that is 0. */
int64_t comic_beam_truncate_workspace(int n_models, int B, int W, int V);
int comic_beam_truncate(const float* logits, const float* weights, int n_models, const int32_t* finished, uint32_t* bits,
                        int words, int B, int W, int V, float temperature, const comic_beam_truncation* truncation,
                        int has_bans, void* workspace, int64_t workspace_bytes, void* stream);
/* out[r,:] = in[(r/W)*W + parent[r], :]   (state re-ordering by parent beam) */
int comic_gather_rows(const float* in, const int32_t* parent, float* out, int rows, int W, int cols,
                      void* stream);
/* beam_search_ops.gather_tree: step_ids/parent_ids/out [T,B,W]; max_len [B]. */
int comic_gather_tree(const int32_t* step_ids, const int32_t* parent_ids, const int32_t* max_len,
                      int32_t* out, int T, int B, int W, int end_id, void* stream);

/* Consensus (minimum-Bayes-risk) selection among the W decoded candidates of every image (csrc/consensus.hip; no
 * counterpart in common/ops_rnn.py): each candidate's mean CIDEr-D similarity to its siblings, directly on token ids, in
 * one launch -- the similarity of the host scorer below (ciderD_scorer.py:52-222) with the siblings as references.
 *   Inputs per image b: ids_tbw[:, b, :], W rows of T ids as comic_gather_tree leaves them (every position after the
 *     first end_id holds end_id); a word length stride >= 1 (1 for `word` tokens, the radix word length for `radix`).
 *   Units.  L = index of the first end_id of a row (T without one), U = L / stride: a trailing partial word is dropped
 *     and <EOS> is never a unit.  Unit i is the tokens [i*stride, (i+1)*stride); an n-gram of order k is k consecutive
 *     units, k = 1..4.
 *   Weights.  g(ng) = 1 without a table.  With one, g(ng) = log(ref_len) - log(max(1, df(ng))), formed in double on the
 *     HOST and stored in the table; an n-gram that the table does not hold gets log_ref_len.  The device evaluates no log.
 *   Vectors.  vec_k[ng] = tf(ng) * g(ng); norm_k = sqrt(sum vec_k^2); len = max(U - 1, 0), the bigram count (the host
 *     scorer's own rule).
 *   Similarity of candidate h against sibling r.  Per order k: val_k = sum over the n-grams of h, in order of first
 *     occurrence, of min(vec_h[ng], vec_r[ng]) * vec_r[ng]; divided by norm_h * norm_r when both are non-zero; times
 *     exp(-(len_h - len_r)^2 / (2 sigma^2)).  sim = 10 * mean_k val_k.
 *   Utility.  u[b, w] = sum_{j != w} pi_j sim(c_w, c_j) / sum_{j != w} pi_j, j ascending.  COMIC_CONSENSUS_UNIFORM:
 *     pi = 1 (the Monte-Carlo estimate over samples; duplicates count once per slot; log_probs is not read and may be
 *     NULL).  COMIC_CONSENSUS_POSTERIOR: pi = softmax over the W slots of log_probs [B, W] (float32; computed in double;
 *     -inf gives 0).  A slot with pi = 0 neither votes nor can be chosen, and its utility is -inf.  A zero denominator
 *     (W = 1, say) gives u = 0.
 *   Result.  utility_bw [B, W] double; best_b [B]: the slot of largest utility among those with pi > 0, the lowest on
 *     ties; 0 when there is none.
 *   Arithmetic.  All float64; every sum is formed by one lane in one fixed order, so two runs give the same bits and no
 *     result depends on how workgroups interleave.
 *   Table.  table_keys_or_null: uint64 keys[table_cap] (0 = empty) beside double table_g[table_cap], open addressing with
 *     linear probing from key & (table_cap - 1); table_cap a power of two, at least twice the number of entries (the
 *     builder's rule; a probe sequence is cut off after table_cap slots).  The key of an n-gram of m = k * stride tokens:
 *     h = splitmix64(m), then h = splitmix64(h ^ uint64(token)) for every token in order (csrc/splitmix.h); a result of
 *     0 is stored and looked up as 1.  INSIDE THE KERNEL TWO N-GRAMS ARE EQUAL WHEN THEIR 64-BIT KEYS ARE: two different
 *     n-grams of an image that collide (probability ~ n^2 / 2^65 for n n-grams) are counted as one.
 *   Limits, refused before any launch (rc 2; the workspace query returns -1): 1 <= W <= 32; U <= 64, i.e.
 *     T <= 64 * stride; 1 <= stride <= 8.
 * workspace: comic_caption_consensus_workspace bytes (0: every intermediate lives in LDS), may be NULL when that is 0. */
#define COMIC_CONSENSUS_UNIFORM 0
#define COMIC_CONSENSUS_POSTERIOR 1
int64_t comic_caption_consensus_workspace(int B, int W, int T, int stride);
int comic_caption_consensus(const int32_t* ids_tbw, int T, int B, int W, int end_id, int stride,
                            const float* log_probs_or_null, int weights_mode, const uint64_t* table_keys_or_null,
                            const double* table_g, int64_t table_cap, double log_ref_len, double sigma,
                            double* utility_bw, int32_t* best_b, void* workspace, int64_t workspace_bytes, void* stream);

/* The SCST reward on the device (csrc/scst_reward.hip): CIDEr-D and per-sentence BLEU-1..4 of the W rollouts of every
 * image (and of an optional baseline rollout) against the image's reference captions, the baseline and the advantage,
 * in one launch -- captionScorer.get_hypo_scores, common/scst/scorers.py:43-171, over ciderD_scorer.py:52-222 and
 * bleu_scorer.py:23-263, on word ids instead of text.
 *   Rollouts.  ids_tbw [T, B, W] int32 as comic_gather_tree leaves them; baseline_ids_t0b_or_null [T0, B] (the greedy
 *     caption) adds a row: W' = W + 1 with it, W without.  baseline_first_eos_b_or_null [B] (comic_decoder_greedy's
 *     first_eos): the greedy loop ends when every image has emitted <EOS> and never writes the rows behind, so with it
 *     only the rows t < min(T0, max_b first_eos[b] + 1) of the baseline ids are read -- what the host reads; NULL: all T0.
 *   Canonical words.  Every rollout is first reduced to the word ids that ops.id_to_caption(skip_unmapped=True) turns
 *     into text.  COMIC_SCST_TOKENS_WORD: the tokens t with 0 <= t < vocab and t != end_id, in order, wherever they stand
 *     (word_len must be 1).  COMIC_SCST_TOKENS_RADIX: the digits 0 <= t < radix_base in order; ONE trailing digit is
 *     dropped when their count is no multiple of word_len, whatever the remainder; groups of word_len digits combine
 *     most significant first, a short last group (word_len > 2) decodes as it stands; word ids >= vocab are dropped.
 *     vocab is the number of word ids the table maps: len(itow), less one where the table lacks the id len(itow) - 1.
 *     All n-gram work is on these word ids, one id per word, for both token types.
 *   References.  refs_brl [B, R, Lr] int32 word ids, negative = padding (skipped); n_refs_b [B], 1 <= n_refs <= R (clamped
 *     to [0, R]; 0 references give NaN).  A word outside the vocabulary carries an extended id >= vocab, one per distinct
 *     string (decoder.RewardVocab): it matches among references and in the table, never a rollout.
 *   Table.  As comic_caption_consensus's, built with one token per word (stride 1) through the same extended ids; NULL:
 *     every n-gram weighs 1.
 *   CIDEr-D of rollout h.  vec, norm and len as comic_caption_consensus states them (len = the bigram count, the host
 *     scorer's own rule), for h and for every reference; val_k(h, r) as there; cider = 10 * (sum_k sum_r val_k(h, r)) / 4
 *     / n_refs, r ascending inside k ascending.
 *   BLEU-1..4 of rollout h.  correct_k = sum over the distinct n-grams of h of min(tf_h, max_r tf_r); guess_k =
 *     max(0, words - k + 1); running product of (correct_k + 1e-15) / (guess_k + 1e-9), bleu_k = product^(1/k); the
 *     reference length is the closest to the rollout's, ties to the shorter; ratio = (words + 1e-15) / (reflen + 1e-9),
 *     and every bleu_k is multiplied by exp(1 - 1 / ratio) when ratio < 1.
 *   Reward.  r = cider * w_cider + bleu_1 * w_bleu4[0] + ... + bleu_4 * w_bleu4[3], added in that order.  A metric whose
 *     largest weight is <= 0 is skipped: it adds nothing and its output is 0.  w_bleu4 is a HOST pointer.
 *   Baseline, for the W rollouts.  COMIC_SCST_BASELINE_NONE: 0.  _ROW: the reward of the baseline row (which must be
 *     given).  _LEAVE_ONE_OUT: (sum_{j != i} r_j) / (W - 1), j ascending; needs W >= 2.
 *   Results.  cider_bw [B, W'], bleu_bw4 [B, W', 4], reward_bw [B, W'] and baseline_bw [B, W] double; advantage_wb
 *     [W, B] float32 = float32(r - baseline), hypothesis-major (row w * B + b): the row order of the SCST update.
 *   Arithmetic.  All float64; every sum is formed by one lane in one fixed order: two runs give the same bits.
 *   Limits, refused before any launch (rc 2; the workspace query returns -1): 1 <= W <= 32, 1 <= R <= 8, 1 <= Lr <= 64,
 *     1 <= word_len <= 8, T and T0 <= 64 * word_len, and the LDS of the geometry -- (W' + R) captions of
 *     Ucap = max(ceil(T / word_len), ceil(T0 / word_len), Lr) words at 72 bytes a word, plus 11 776 bytes -- within a
 *     workgroup's 160 KiB.  comic_scst_reward_workspace returns those LDS bytes (no global workspace is needed).
 *
 * comic_scst_coefficients: the two float32 blocks that comic_decoder_train_step's SCST loss reads, formed on the device
 * from the staged mask wmask_rt [rows, T] and advantage_r [rows] with the float32 operations of the host formula
 * (Decoder.train_step): den = sum_t wmask + 1e-12f; rb = adv / rows; row_scale = rb / den; coef = wmask / den * rb.
 * Correctly rounded division, no contraction: bit-equal to numpy. */
#define COMIC_SCST_TOKENS_WORD 0
#define COMIC_SCST_TOKENS_RADIX 1
#define COMIC_SCST_BASELINE_NONE 0
#define COMIC_SCST_BASELINE_ROW 1
#define COMIC_SCST_BASELINE_LEAVE_ONE_OUT 2
int64_t comic_scst_reward_workspace(int B, int W, int has_baseline_row, int T, int T0, int word_len, int R, int Lr);
int comic_scst_reward(const int32_t* ids_tbw, int T, int B, int W, const int32_t* baseline_ids_t0b_or_null, int T0,
                      const int32_t* baseline_first_eos_b_or_null, int token_mode, int end_id, int radix_base, int word_len, int vocab, const int32_t* refs_brl,
                      const int32_t* n_refs_b, int R, int Lr, const uint64_t* table_keys_or_null, const double* table_g,
                      int64_t table_cap, double log_ref_len, double sigma, double w_cider, const double* w_bleu4,
                      int baseline_mode, double* cider_bw, double* bleu_bw4, double* reward_bw, double* baseline_bw,
                      float* advantage_wb, void* stream);
int comic_scst_coefficients(const float* wmask_rt, const float* advantage_r, int rows, int T, float* coef_rt,
                            float* row_scale_rt, void* stream);

/* ------------------------------------------------------------------------- */
/* Optimiser (model_base.py:852-883; tf.train.AdamOptimizer ApplyAdam, TF-1.9)  */
/* ------------------------------------------------------------------------- */
/* g_eff = g*gscale + l2*w; m += (g_eff-m)(1-b1); v += (g_eff^2-v)(1-b2);
 * w -= lr_t*m/(sqrt(v)+eps), lr_t = lr*sqrt(1-b2^t)/(1-b1^t) computed by the caller. */
int comic_adam_tf(float* w, const float* g, float* m, float* v, int64_t n, float lr_t, float beta1,
                  float beta2, float eps, float l2, float gscale, void* stream);
/* Legacy encoder head (`--legacy`, model_base.py:80-91): ops.layer_norm_activate('LN_tanh', squeeze(net), tanh)
 * (common/ops.py:241-275: tf.contrib.layers.layer_norm over the last axis, eps 1e-12, center + scale) followed by
 * ops.linear('im_embed', 1024, no bias) = comic_gemm_f32.  y = tanh(xhat*gamma + beta), xhat = (x-mean)*rsqrt(var+eps)
 * (kept for the backward).  comic_ln_tanh_bwd_rows writes the per-row terms of d gamma / d beta
 * (dy*(1-y^2)*xhat and dy*(1-y^2)); their column sums (comic_colsum) are the parameter gradients.  The head is never
 * back-propagated into the CNN: train.py:241-249 refuses cnn_finetune / scst with --legacy. */
int comic_ln_tanh_fwd(const float* x, const float* gamma, const float* beta, float* y, float* xhat, int B, int C,
                      float eps, void* stream);
int comic_ln_tanh_bwd_rows(const float* dy, const float* y, const float* xhat, float* pgamma, float* pbeta, int B,
                           int C, void* stream);
/* tf.train.MomentumOptimizer(momentum 0.9, use_nesterov=False) (model_base.py:867-880; ApplyMomentum, TF-1.9):
 * g_eff = g*gscale + l2*w; accum = momentum*accum + g_eff; w -= lr*accum. */
int comic_momentum_tf(float* w, const float* g, float* accum, int64_t n, float lr, float momentum, float l2,
                      float gscale, void* stream);
/* The same updates, skipped ON THE DEVICE (w, m, v / accum untouched) when skip_flag[0] != 0: the optimiser step behind a
 * training step that comic_decoder_train_step voided (comic_decoder_params::status of the gradient table).  NULL = never
 * skip. */
int comic_adam_tf_gated(float* w, const float* g, float* m, float* v, int64_t n, float lr_t, float beta1, float beta2,
                        float epsilon, float l2, float gscale, const float* skip_flag, void* stream);
int comic_momentum_tf_gated(float* w, const float* g, float* accum, int64_t n, float lr, float momentum, float l2,
                            float gscale, const float* skip_flag, void* stream);
/* The gated updates with tf.train.ExponentialMovingAverage's shadow of w kept in the same launch (`--ema_decay`): after the
 * new w[i] is formed,  shadow[i] = shadow[i] + (w_new - shadow[i]) * one_minus_decay  (TF's shadow -= (1 - decay) *
 * (shadow - var), applied to the UPDATED variable; one_minus_decay = 1 - min(decay, (1 + n) / (10 + n)) computed by the
 * caller, 0 < one_minus_decay <= 1).  w, m, v / accum get the bits of the gated forms; a voided step (skip_flag[0] != 0)
 * leaves the shadow untouched as well.  n > 0 is any element count (callers pass ranges); shadow must not be NULL. */
int comic_adam_tf_ema(float* w, const float* g, float* m, float* v, int64_t n, float lr_t, float beta1, float beta2,
                      float epsilon, float l2, float gscale, const float* skip_flag, float* shadow, float one_minus_decay,
                      void* stream);
int comic_momentum_tf_ema(float* w, const float* g, float* accum, int64_t n, float lr, float momentum, float l2,
                          float gscale, const float* skip_flag, float* shadow, float one_minus_decay, void* stream);
/* Gradual magnitude pruning (`--prune_sparsity`, Zhu & Gupta 2017; csrc/prune.hip).  The MASK of a flat buffer of n_total
 * floats is ceil(n_total / 32) uint32 words: bit i % 32 of word i / 32 is 1 while element i is live; padding and variables
 * that are never pruned keep their 1.  SEGMENTS: n_seg records of three int64 on the device, (first element, elements, group),
 * ascending by first element and not overlapping -- the prunable variables without their alignment padding; group in
 * [0, n_groups).  A segment that does not lie inside [0, n_total) or names an unknown group is ignored.
 *
 * comic_prune_select: one mask event.  For every group g the elements of its segments are ordered: already pruned elements
 * first, then the live ones by ascending |w| compared on the IEEE bits of |w| (-0.0 == +0.0, -x == +x, denormals in their
 * place), ties by lowest flat index; the first targets[g] (int64 on the device, clamped to the group's size) of that
 * order are pruned afterwards.  A target that is not above the group's pruned count changes nothing: masks are sticky.  A
 * newly pruned element gets its bit cleared and +0.0f in w, m, v and (when not NULL) shadow; every other bit and float of
 * the five buffers keeps its bits.  Exact and independent of the order of execution (integer histograms, no float atomics,
 * no sort): two runs on the same input give the same bytes.  workspace: comic_prune_workspace_bytes(n_total, n_seg,
 * n_groups) bytes (-1: bad arguments), cleared by the call.
 * comic_prune_mask_buffer: x[i] = +0.0f where bit first_bit + i of the mask is clear, i < n (the gradient in front of
 * comic_clip_by_norm; the slots of a run started with --prune_keep_zeros).
 * comic_prune_mask_from_zeros: the mask of --prune_keep_zeros: all ones, then bit i cleared where w[i] == 0 inside a segment
 * (the groups of the table are not read). */
int64_t comic_prune_workspace_bytes(int64_t n_total, int n_seg, int n_groups);
int comic_prune_select(float* w, uint32_t* mask, int64_t n_total, const int64_t* segments, int n_seg,
                       const int64_t* targets, int n_groups, float* m, float* v, float* shadow, void* workspace,
                       int64_t workspace_bytes, void* stream);
int comic_prune_mask_buffer(float* x, const uint32_t* mask, int64_t first_bit, int64_t n, void* stream);
int comic_prune_mask_from_zeros(const float* w, uint32_t* mask, int64_t n_total, const int64_t* segments, int n_seg,
                                void* stream);
/* The gated (shadow == NULL; one_minus_decay unread) or EMA (shadow != NULL) updates under such a mask: element i of the range
 * is element first + i of the masked buffer (first >= 0; a range of DataParallel.chunk_bounds starts on a word boundary, any
 * other start works as well).  A live element gets the bits of comic_*_tf_gated / comic_*_tf_ema; a pruned one is left as the
 * mask event wrote it, +0.0f in w, m, v / accum and shadow, whatever its gradient is; a voided step leaves everything. */
int comic_adam_tf_masked(float* w, const float* g, float* m, float* v, int64_t n, float lr_t, float beta1, float beta2,
                         float epsilon, float l2, float gscale, const float* skip_flag, float* shadow,
                         float one_minus_decay, const uint32_t* mask, int64_t first, void* stream);
int comic_momentum_tf_masked(float* w, const float* g, float* accum, int64_t n, float lr, float momentum, float l2,
                             float gscale, const float* skip_flag, float* shadow, float one_minus_decay,
                             const uint32_t* mask, int64_t first, void* stream);
/* Gradient clipping of `--clip_gradient_norm` (train.py:137 -> model_base.py:394-401: slim.learning.create_train_op(
 * clip_gradient_norm=c) = clip_gradient_norms [TF-1.9 slim]: tf.clip_by_norm on EVERY variable's gradient by that tensor's
 * own L2 norm, after the gradient multipliers).  The clipped quantity is g_eff = g*gscale + l2*w (the L2 term is part of
 * the reference's loss; gscale carries the data-parallel 1/W and the CNN multiplier): g_eff * clip / max(||g_eff||, clip).
 * In place on g, such that the optimiser's own g*gscale + l2*w yields the clipped g_eff.  chunks: n_chunks records of five
 * int64 on the device -- (variable, first element, elements, first chunk of the variable, chunks of the variable), a
 * variable cut into pieces of <= 8192 elements; partial: n_chunks floats of scratch.  Sums run in a fixed order.  skip_flag
 * as in comic_adam_tf_gated. */
int comic_clip_by_norm(float* g, const float* w, const int64_t* chunks, int n_chunks, float l2, float gscale,
                       float clip_norm, float* partial, const float* skip_flag, void* stream);
/* Test aid: n_workgroups workgroups (256 threads) that stay resident for about `microseconds` each (bounded spin on the
 * 100 MHz clock) -- what a collective's kernels do to some CUs while a training step runs beside them. */
int comic_debug_occupy_cus(int n_workgroups, int microseconds, void* stream);
/* out[j] = sum_i in[i*cols + j]  (deterministic column sums; parameter-partial reduce) */
int comic_colsum(const float* in, float* out, int rows, int cols, float beta, void* stream);
int comic_axpy(float* y, const float* x, float a, int64_t n, void* stream);

/* ------------------------------------------------------------------------- */
/* Native decoder executors                                                   */
/* ------------------------------------------------------------------------- */
typedef struct comic_decoder_desc {
  int32_t D, E, A, V, C, Cg, H, M;     /* rnn, word, attention, softmax, fm ch, im_embed, heads, map */
  int32_t Cv;                          /* value channels (D, or C when projection is none) */
  int32_t fm_projection;               /* 0 none, 1 independent, 2 tied */
  int32_t method, prob;                /* as comic_attn_desc */
  int32_t context_layer;               /* attn_context_layer */
  int32_t init_method;                 /* 0 first_input, 1 project_hidden */
  int32_t start_id, end_id;
  float keep_in, keep_out, keep_alpha; /* 1.0 disables the dropout */
  float map_loss_scale;
  uint32_t flags;                      /* COMIC_DEC_* executor switches, 0 = every fast path on (A/B measurements and tests;
                                          results agree to fp32 summation order).  The library reads no environment. */
  float length_penalty_weight;         /* comic_decoder_beam only: BeamSearchDecoder(length_penalty_weight) -- candidates
                                          are ranked by total / ((5 + length) / 6)^w (ops_rnn.py:96, infer.py:65); 0 = none */
  int32_t cell;                        /* COMIC_CELL_*: --rnn_name (src/model_base.py:606-632) */
} comic_decoder_desc;
#define COMIC_CELL_LSTM 0               /* tf.contrib.rnn.BasicLSTMCell: K [E+A+D][4D], b [4D] */
#define COMIC_CELL_LN_LSTM 1            /* tf.contrib.rnn.LayerNormBasicLSTMCell: K [E+A+D][4D], no bias, cell_ln */
#define COMIC_CELL_GRU 2                /* tf.contrib.rnn.GRUCell: K [E+A+D][2D] + b [2D] (gates), K_c [E+A+D][D] + b_c [D] (candidate) */
#define COMIC_DEC_NO_PERSIST 1u         /* time loops as per-step launches (forward and backward; greedy too) */
#define COMIC_DEC_NO_PERSIST_BWD 2u     /* backward time loop as per-step launches */
#define COMIC_DEC_NO_FUSED_STEP 4u      /* split-K GEMM + element-wise kernel chain instead of the fused step kernels */
#define COMIC_DEC_NO_SPLIT_ATTN_BWD 8u  /* one attention-backward workgroup per batch row */
#define COMIC_DEC_ONE_LANE 16u          /* no second stream inside the training executor */
#define COMIC_DEC_EXACT_GEMM 32u        /* exact-fp32 MFMA for the time-batched products (no hi/lo-split bf16) */
#define COMIC_DEC_STAMPS 64u            /* diagnostic phase clocks of the persistent loops (host sync per launch) */
#define COMIC_DEC_PHASE_FWD 512u        /* comic_decoder_train_step: only the part that needs no loss coefficient (forward to the logits) */
#define COMIC_DEC_PHASE_BWD 1024u       /* ... only the rest (loss, backward), over the SAME workspace and arguments as the forward call */
#define COMIC_DEC_NO_GROUP_GEMM 2048u    /* comic_decoder_train_step: the products outside the time loops as separate launches on two lanes
                                           instead of grouped launches (comic_gemm_group) */
#define COMIC_DEC_INJECT_TIMEOUT 8192u  /* fault injection (tests): THIS comic_decoder_train_step call, if it runs a persistent loop, reports a loop
                                           timeout (NaN loss_rows[0] / map_loss, zero gradients, status words raised) although its kernels completed */
#define COMIC_DEC_BWD_OWN_ROWS 4096u    /* persistent backward loop in its own-rows form (the form of memories of more than 64 rows) whatever M is */
#define COMIC_DEC_NO_LSTM_STREAM 256u   /* decode steps at > 32 rows with the per-row-tile fused LSTM kernel instead of the streaming one */
#define COMIC_DEC_NO_BEAM_LOGITS 128u   /* beam step as GEMM + statistics + chunk top-k + merge (large V) / comic_beam_step's kernel (small V)
                                           instead of the streaming logits + top-k launch / the register-resident small step */

/* Parameter (or gradient) table; every pointer is a view into one flat fp32 buffer. */
typedef struct comic_decoder_params {
  float *W_init, *K, *b, *W_m, *W_v, *W_q, *v, *ln_g, *ln_b, *tau, *W_a, *W_o, *b_o, *emb;
  float* cell_ln;   /* LN_LSTM: ten [D] vectors gamma, beta of the scopes input, transform, forget, output, state, in that
                       order, (D + 63) / 64 * 64 floats apart; NULL otherwise */
  float *K_c, *b_c; /* GRU: candidate kernel and bias; NULL otherwise */
  float* status;    /* optional (may be NULL), one float behind the flat buffer.  In the GRADIENT table: comic_decoder_train_step
                       writes 1 when it voided the step (a bounded wait of a persistent loop expired), else 0 -- the word the
                       gated optimiser entries read; it lies inside the all-reduced buffer, so under data parallelism every
                       rank sees a non-zero sum and skips the same update.  In the PARAMETER table: a sticky count of voided
                       steps (incremented, never cleared by the library) for the host to read at its log points. */
} comic_decoder_params;

/* Workspace size in bytes for a training step at (B, T, M) / a decode at rows=B*W. */
int64_t comic_decoder_train_workspace(const comic_decoder_desc* d, int B, int T);
int64_t comic_decoder_infer_workspace(const comic_decoder_desc* d, int rows, int max_steps);

/* One teacher-forced forward + backward (CaptionModel train graph: src/model.py:44-59;
 * rnn_decoder_training ops_rnn.py:183-243; losses model_base.py:325-405).
 *   fm [B,M,C], im_embed [B,Cg] fp32; inputs_bt/targets_bt [B,T] int32; wmask/coef [B,T];
 *   lens [B] int32 (device) and Tp = max(lens) (host);
 *   masks (may be NULL when the keeps are 1): init_in [B,E+A], in [Tp,B,E+A],
 *   out [Tp,B,D], alpha [Tp,B,H,M].
 * Outputs: logits [T,B,V] (time-major), ids [T,B], attn history [Tp,B,H,M], loss_rows [T*B],
 *   map_loss (1 float), grads (no L2), dfm [B,M,C] / dim_embed [B,Cg] (may be NULL).
 * The forward and the backward time loop each run as ONE persistent launch per 64 batch rows when the shape allows
 * (D = 512, B <= 256, no context layer, M <= 64 or tied keys/values and M <= 256; backward: tied keys/values, softmax,
 * M <= 256; a device with >= 256 CUs), as
 * per-step launches otherwise: same results to fp32 summation order (comic_decoder_train_path tells which).  If a
 * bounded wait inside a persistent loop ever expires, the step's results are void and the call says so in its
 * outputs: loss_rows[0] and map_loss[0] are NaN (the sequence loss reduced from loss_rows is then NaN too) and every
 * gradient (grads, dfm, dim_embed) is zero, so an optimiser step issued without a host check applies no gradient. */
int comic_decoder_train_step(const comic_decoder_desc* d, const comic_decoder_params* p,
                             const comic_decoder_params* grads, const float* fm,
                             const float* im_embed, const int32_t* inputs_bt,
                             const int32_t* targets_bt, const float* wmask_bt, const float* coef_bt,
                             const int32_t* lens, int B, int T, int Tp, const float* mask_init_in,
                             const float* mask_in, const float* mask_out, const float* mask_alpha,
                             float* logits_tb, int32_t* ids_tb, float* attn_hist, float* loss_rows,
                             float* map_loss, float* dfm, float* dim_embed, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* Soft-target XE training: label smoothing and distillation from a teacher's top-K table.  For a live token row with
 * logits z, p = softmax(z), target y, eps = smoothing in [0, 1), lam = teacher_weight in [0, 1], eps + lam <= 1:
 *   q_T(v)    = sum_k [ids_k = v] probs_k / S,  S = sum_k probs_k    (the table holds raw probabilities; the loss
 *                                                                      renormalises the kept mass)
 *   q         = (1 - eps - lam) e_y + eps / V + lam q_T
 *   loss_rows = wmask (lse(z) - sum_v q_v z_v)     the cross-entropy H(q, p), NOT the KL divergence: they differ by the
 *                                                  entropy of q, a constant in the parameters
 *   nll_rows  = wmask (lse(z) - z_y)               the hard loss, so that logged perplexities stay comparable
 *   dlogits   = (p - q) coef                       (the student's temperature is 1; no tau^2 factor)
 * Rows with t >= lens[b], the arg-max ids, coef and wmask: as in comic_xent_fwd_bwd.  The ids of a table row are
 * distinct and in [0, V), its probs >= 0 with S > 0 on live rows; rows past lens are never read.
 *   ids_tbk / probs_tbk [T,B,K] (device; both NULL with teacher_weight 0: label smoothing alone), 1 <= K <= min(32, V);
 *   nll_rows [T*B] (device) or NULL. */
#define COMIC_SOFT_MAX_K 32
typedef struct comic_soft_targets {
  float smoothing;
  float teacher_weight;
  int K;
  const int32_t* ids_tbk;
  const float* probs_tbk;
  float* nll_rows;
} comic_soft_targets;

/* comic_decoder_train_step against soft targets.  soft == NULL IS comic_decoder_train_step: the same launches, the same
 * bits.  With a record, the ONE launch between the logits product and the backward is the soft loss (csrc/xent_soft.hip)
 * and, where the map loss rode on that launch, its two own launches follow (the partial sums and their combination in
 * piece order: the bits of the fused form); everything else of the step is unchanged.  With COMIC_DEC_PHASE_FWD /
 * _BWD the record matters in the BWD call only.  The coefficients must be the XE step's: soft targets and SCST
 * rewards do not combine. */
int comic_decoder_train_step_soft(const comic_decoder_desc* d, const comic_decoder_params* p,
                                  const comic_decoder_params* grads, const float* fm,
                                  const float* im_embed, const int32_t* inputs_bt,
                                  const int32_t* targets_bt, const float* wmask_bt, const float* coef_bt,
                                  const int32_t* lens, int B, int T, int Tp, const float* mask_init_in,
                                  const float* mask_in, const float* mask_out, const float* mask_alpha,
                                  float* logits_tb, int32_t* ids_tb, float* attn_hist, float* loss_rows,
                                  float* map_loss, float* dfm, float* dim_embed, void* workspace,
                                  int64_t workspace_bytes, void* stream, const comic_soft_targets* soft);

/* The soft loss alone, on its own operands (the launch of comic_decoder_train_step_soft): logits [t_stride,B,V] of
 * which t_rows steps are live, the [B,t_stride] tables of comic_xent_fwd_bwd, d logits rows ld_dl >= V floats apart
 * (columns V .. ld_dl-1 are written as zeros). */
int comic_xent_soft(float* logits, const int32_t* targets_bt, const float* coef_bt, const float* wmask_bt,
                    const int32_t* lens, float* loss_rows, float* nll_rows, float* dlogits, int ld_dl,
                    int32_t* ids_tb, int t_rows, int t_stride, int B, int V, float smoothing, float teacher_weight,
                    int K, const int32_t* ids_tbk, const float* probs_tbk, void* stream);

/* The teacher's table: for every live row (t < Tp and t < lens[b]) of n <= 8 members' time-major logits [T,B,V],
 *   pbar(v) = sum_m weights[m] softmax(z_m / temperature)(v),
 * the K largest pbar ordered by (pbar descending, id ascending) -- ties at the boundary go to the lowest id -- as
 * ids [T,B,K] and probs [T,B,K] = those pbar values.  Other rows get ids 0 .. K-1 and probs 0.  logits and weights are
 * HOST arrays of n entries (device pointers / weights >= 0 summing to 1); 1 <= K <= min(32, V); temperature in (0, inf).
 * One workgroup per row holds pbar in LDS: V * 4 + 2048 bytes must fit 160 KB (V <= 40448), a larger V is refused.  No
 * atomics, fixed summation orders: two runs give the same bits. */
int comic_teacher_topk(const float* const* logits, const float* weights, int n, const int32_t* lens, int B, int T, int Tp,
                       int V, float temperature, int K, int32_t* ids, float* probs, void* stream);

/* Which form of the time loops the LAST comic_decoder_train_step of this thread used: bit 0 = forward loop as one
 * persistent launch (csrc/decoder_persist.hip), bit 1 = backward loop as one persistent launch
 * (csrc/decoder_persist_bwd.hip); 0 = per-step launches.  The choice depends on the shape (D = 512, B <= 64, ...), the
 * device (one workgroup per CU must be resident) and the COMIC_PERSIST / COMIC_PERSIST_BWD switches. */
int comic_decoder_train_path(void);
/* 1 when the LAST comic_decoder_greedy of this thread ran its loop as one persistent launch (D = 512, B <= 64,
 * V <= 512, no context layer, a device with enough CUs, COMIC_PERSIST != 0), 0 for per-step launches. */
int comic_decoder_greedy_path(void);
/* Paths of the LAST comic_decoder_beam of this thread, a bit mask: 1 = projection + top-k as the streaming launch over
 * a packed W_o (csrc/beam_logits.hip: D % 128 == 0, V >= 4096, batch * beam <= 256, beam <= 8, fused step available)
 * instead of the GEMM + statistics + top-k launches; 2 = the LSTM step as one streaming pass over the packed kernel
 * (csrc/lstm_stream.hip: 33 ... 256 rows) instead of the per-row-tile fused kernel; 4 = small vocabulary (V <= 1024, beam
 * <= 8): the entry's beam step with a beam's logits held in a wave's registers (beam_step_small_kernel) instead of
 * comic_beam_step's kernel + the all-finished launch. */
int comic_decoder_beam_path(void);

/* Caption scoring: log p(caption | image) of given captions, forward only -- the teacher-forced half of
 * rnn_decoder_training (common/ops_rnn.py:183-243) and the per-token terms of the sequence loss (_train_caption_model,
 * src/model_base.py:325-347: sparse softmax cross-entropy times the caption mask) WITHOUT their reduction to one number.
 * The forward (memory projections, rnn init, time loop) is the code of comic_decoder_train_step with the dropout masks
 * absent; no gradient table is taken, nothing is filled for a backward, and the workspace holds none of the backward's
 * blocks (comic_decoder_score_workspace < comic_decoder_train_workspace).  Same cells, alignment methods, probability
 * functions, projection modes and COMIC_DEC_* switches as the training step (the keeps and the phase / fault-injection
 * flags of the descriptor are ignored).
 *   inputs as comic_decoder_train_step: fm [B,M,C], im_embed [B,Cg], inputs_bt / targets_bt [B,T] int32, wmask_bt [B,T],
 *   lens [B] int32 (device), Tp = max(lens) (host).
 * Outputs: token_logp_tb [T,B] = wmask * (logit[target] - logsumexp(y W_o + b_o)), exactly 0 where wmask == 0 or
 *   t >= lens[b]; caption_logp [B] = the float32 sum of a caption's tokens in t order; attn_hist [Tp,B,H,M] or NULL.
 * Deterministic: partial results are combined in a fixed order, no atomics.  If a bounded wait of the persistent forward
 * loop expires, every output is NaN. */
int64_t comic_decoder_score_workspace(const comic_decoder_desc* d, int B, int T);
int comic_decoder_score(const comic_decoder_desc* d, const comic_decoder_params* p, const float* fm, const float* im_embed,
                        const int32_t* inputs_bt, const int32_t* targets_bt, const float* wmask_bt, const int32_t* lens,
                        int B, int T, int Tp, float* token_logp_tb /*[T,B]*/, float* caption_logp /*[B]*/,
                        float* attn_hist /*[Tp,B,H,M] or NULL*/, void* workspace, int64_t workspace_bytes, void* stream);
/* Paths of the LAST comic_decoder_score of this thread, a bit mask: bit 0 = forward loop as one persistent launch
 * (csrc/decoder_persist.hip, the conditions of comic_decoder_train_path bit 0); bit 1 = streaming projection over the
 * packed W_o (csrc/score_logits.hip: D % 128 == 0, V >= 4096, COMIC_DEC_NO_BEAM_LOGITS clear) -- no logits in memory --
 * instead of the GEMM into workspace + one wave per row. */
int comic_decoder_score_path(void);   /* bit 0: forward loop persistent; bit 1: streaming projection (no logits in memory) */

/* Greedy decode (rnn_decoder_search, ops_rnn.py:115-180): runs `max_steps` steps on the
 * device without host sync; ids [max_steps,B], attn [max_steps,B,H,M]; finished-at step per
 * row in first_eos [B] (max_steps when no EOS).  The host trims to the executed length. */
int comic_decoder_greedy(const comic_decoder_desc* d, const comic_decoder_params* p, const float* fm,
                         const float* im_embed, int B, int max_steps, int32_t* ids_tb,
                         float* logits_tb, float* attn_hist, int32_t* first_eos, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* Sampled decode (rnn_decoder_search(greedy_search=False), ops_rnn.py:158-166: SampleEmbeddingHelper [TF-1.9]: the next
 * token is a draw of Categorical(logits), fed back through the embedding; finished when it is EOS).  The draw is
 * argmax(logits + g) with Gumbel noise g = -log(-log u) supplied by the caller (gumbel_tb [max_steps,B,V]), i.e. the
 * random stream is the caller's; logits_tb stays the undisturbed projection (BasicDecoder's rnn_output).  Per-step
 * launches; outputs as comic_decoder_greedy. */
int comic_decoder_sample(const comic_decoder_desc* d, const comic_decoder_params* p, const float* fm,
                         const float* im_embed, int B, int max_steps, const float* gumbel_tb, int32_t* ids_tb,
                         float* logits_tb, float* attn_hist, int32_t* first_eos, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* Beam search (rnn_decoder_beam_search, ops_rnn.py:49-112).  fm/im_embed are UN-tiled
 * [B,...]; tiling by W happens inside (model_base.py:127-131).  Outputs, all [max_steps,B,W]:
 * step_ids, parent_ids, scores; final lengths [B,W] (int64), finished [B,W];
 * attn_hist [max_steps, B*W, H*M] (un-sorted; sort on host with gather_tree_from_array).
 * The loop always issues max_steps steps (no host sync); steps_executed (device int32)
 * receives the step count after which every beam was finished, i.e. the length the
 * reference's dynamic_decode would have produced; later steps are identity and ignored. */
int comic_decoder_beam(const comic_decoder_desc* d, const comic_decoder_params* p, const float* fm,
                       const float* im_embed, int B, int W, int max_steps, int32_t* step_ids,
                       int32_t* parent_ids, float* scores, int64_t* lengths, int32_t* finished,
                       float* attn_hist, int32_t* steps_executed, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* Ensemble beam search (extends rnn_decoder_beam_search, common/ops_rnn.py:49-112): ONE beam whose step distribution is
 * the weighted mean of n_models members' distributions (comic_beam_step_ensemble).  descs / params: arrays of n_models
 * entries; fms / im_embeds / attn_hists: HOST arrays of n_models device pointers (member m's fm [B,M_m,C_m], im_embed
 * [B,Cg_m], attn_hist [max_steps, B*W, H_m*M_m] or NULL when its alignments are not wanted; attn_hists itself may be
 * NULL); weights [n_models] on the host.  Members may differ in D, E, H, M, C, cell and attention method and must agree
 * in V, start_id and end_id; length_penalty_weight is descs[0]'s.  Every member runs its own wrapper step on the shared
 * ids / parents of the step before; outputs, early exit through steps_executed and the untouched rows past it as
 * comic_decoder_beam.  workspace: comic_decoder_beam_ensemble_workspace(descs, n_models, B*W, max_steps) bytes. */
int64_t comic_decoder_beam_ensemble_workspace(const comic_decoder_desc* descs, int n_models, int rows, int max_steps);
int comic_decoder_beam_ensemble(const comic_decoder_desc* descs, const comic_decoder_params* params,
                                const float* const* fms, const float* const* im_embeds, const float* weights,
                                int n_models, int B, int W, int max_steps, int32_t* step_ids, int32_t* parent_ids,
                                float* scores, int64_t* lengths, int32_t* finished, float* const* attn_hists,
                                int32_t* steps_executed, void* workspace, int64_t workspace_bytes, void* stream);

/* Constrained beam search (extends rnn_decoder_beam_search, common/ops_rnn.py:49-112): comic_decoder_beam_ensemble -- the
 * same loop; a single decoder is n_models == 1 with weight 1 -- whose every step first builds the beams' ban masks
 * (comic_beam_bans) and then ranks through them (comic_beam_step_constrained).  Besides the rules of the struct:
 * min_length < max_steps, V <= 65 536 and V >= W + n_suppress + 1 + max_steps, so that a live beam always keeps W
 * candidates and a banned token is never selected.  Everything else, outputs included, as comic_decoder_beam_ensemble.
 * workspace: comic_decoder_beam_constrained_workspace(descs, n_models, B*W, max_steps) bytes. */
int64_t comic_decoder_beam_constrained_workspace(const comic_decoder_desc* descs, int n_models, int rows, int max_steps);
int comic_decoder_beam_constrained(const comic_decoder_desc* descs, const comic_decoder_params* params,
                                   const float* const* fms, const float* const* im_embeds, const float* weights,
                                   int n_models, int B, int W, int max_steps, const comic_beam_constraints* constraints,
                                   int32_t* step_ids, int32_t* parent_ids, float* scores, int64_t* lengths,
                                   int32_t* finished, float* const* attn_hists, int32_t* steps_executed, void* workspace,
                                   int64_t workspace_bytes, void* stream);

/* Diverse beam search (extends rnn_decoder_beam_search, common/ops_rnn.py:49-112): comic_decoder_beam_ensemble /
 * comic_decoder_beam_constrained -- the same loop; a single decoder is n_models == 1 with weight 1 -- whose beams start
 * with the first slot of every group live and whose every step ranks under `groups` (comic_beam_step_diverse, the rule
 * at comic_beam_groups).  constraints may be NULL; given, their rules hold unchanged (V >= W + n_suppress + 1 +
 * max_steps, ...).  groups must not be NULL: 1 <= groups <= W, W % groups == 0, diversity finite and >= 0, W / groups <= V.
 * Slot g * (W / groups) of the outputs is group g's best.  Everything else as comic_decoder_beam_ensemble.
 * workspace: comic_decoder_beam_diverse_workspace(descs, n_models, B*W, max_steps, constrained) bytes, constrained != 0
 * when constraints are given (the constrained layout), else the ensemble's. */
int64_t comic_decoder_beam_diverse_workspace(const comic_decoder_desc* descs, int n_models, int rows, int max_steps,
                                             int constrained);
int comic_decoder_beam_diverse(const comic_decoder_desc* descs, const comic_decoder_params* params,
                               const float* const* fms, const float* const* im_embeds, const float* weights, int n_models,
                               int B, int W, int max_steps, const comic_beam_constraints* constraints,
                               const comic_beam_groups* groups, int32_t* step_ids, int32_t* parent_ids, float* scores,
                               int64_t* lengths, int32_t* finished, float* const* attn_hists, int32_t* steps_executed,
                               void* workspace, int64_t workspace_bytes, void* stream);

/* Sampled decode (extends rnn_decoder_beam_search, common/ops_rnn.py:49-112): comic_decoder_beam_ensemble /
 * comic_decoder_beam_constrained -- the same loop; a single decoder is n_models == 1 with weight 1 -- whose W slots all
 * start live with log-probability 0 and whose step t ranks under `sampling` (comic_beam_step_sampled, the rule at
 * comic_beam_sampling): W samples per image, `scores` [max_steps][B][W] the chains' running log p(caption | image),
 * parent_ids the slot itself.  constraints may be NULL; given, their rules hold unchanged.  sampling and its seed_dev
 * must not be NULL; descs[0].length_penalty_weight must be 0.  Everything else as comic_decoder_beam_ensemble.
 * workspace: comic_decoder_beam_sampled_workspace(descs, n_models, B*W, max_steps, constrained) bytes, constrained != 0
 * when constraints are given. */
int64_t comic_decoder_beam_sampled_workspace(const comic_decoder_desc* descs, int n_models, int rows, int max_steps,
                                             int constrained);
int comic_decoder_beam_sampled(const comic_decoder_desc* descs, const comic_decoder_params* params,
                               const float* const* fms, const float* const* im_embeds, const float* weights, int n_models,
                               int B, int W, int max_steps, const comic_beam_constraints* constraints,
                               const comic_beam_sampling* sampling, int32_t* step_ids, int32_t* parent_ids, float* scores,
                               int64_t* lengths, int32_t* finished, float* const* attn_hists, int32_t* steps_executed,
                               void* workspace, int64_t workspace_bytes, void* stream);
/* Sampled decode under a truncation (extends rnn_decoder_beam_search, common/ops_rnn.py:49-112):
 * comic_decoder_beam_sampled -- the same loop -- with one more launch per step, between the ban bookkeeping and the
 * sampled step: comic_beam_truncate under sampling->temperature, on the constraints' mask when there are constraints,
 * else on a mask of its own.  The sampled step then ranks through that mask.  `scores` stay the chains' running
 * UNTRUNCATED log p(caption | image).  truncation must not be NULL and must do something: refused are top_k < 0,
 * top_p NaN or <= 0, both stages off (top_k == 0 or >= V, with top_p >= 1) and V > 65 536.  Everything else as
 * comic_decoder_beam_sampled.  workspace: comic_decoder_beam_truncated_workspace bytes. */
int64_t comic_decoder_beam_truncated_workspace(const comic_decoder_desc* descs, int n_models, int rows, int max_steps,
                                               int constrained);
int comic_decoder_beam_truncated(const comic_decoder_desc* descs, const comic_decoder_params* params,
                                 const float* const* fms, const float* const* im_embeds, const float* weights, int n_models,
                                 int B, int W, int max_steps, const comic_beam_constraints* constraints,
                                 const comic_beam_sampling* sampling, const comic_beam_truncation* truncation,
                                 int32_t* step_ids, int32_t* parent_ids, float* scores, int64_t* lengths, int32_t* finished,
                                 float* const* attn_hists, int32_t* steps_executed, void* workspace,
                                 int64_t workspace_bytes, void* stream);

/* Beam search with required words (extends rnn_decoder_beam_search, common/ops_rnn.py:49-112):
 * comic_decoder_beam_ensemble / comic_decoder_beam_constrained -- the same loop; a single decoder is n_models == 1 with
 * weight 1 -- whose initial state comes from the table's padding rows and whose every step first runs the bookkeeping
 * (comic_beam_required_table) and then ranks by banks (comic_beam_step_required; the rule at comic_beam_required).  required and
 * req (device, int32 [B][n_words][stride]) must not be NULL.  constraints may be NULL; given, their rules hold with the
 * head-room extended by the specials: V >= W + n_suppress + 1 + max_steps + 4.  The length penalty of descs[0] applies.
 * groups (more than one group) and sampling do not combine with required words: anything but NULL / one group is refused.
 * Slot c * (W / banks) of the outputs is bank c's best.  Everything else as comic_decoder_beam_ensemble.
 * workspace: comic_decoder_beam_required_workspace(descs, n_models, B*W, max_steps, constrained) bytes. */
int64_t comic_decoder_beam_required_workspace(const comic_decoder_desc* descs, int n_models, int rows, int max_steps,
                                              int constrained);
int comic_decoder_beam_required(const comic_decoder_desc* descs, const comic_decoder_params* params,
                                const float* const* fms, const float* const* im_embeds, const float* weights, int n_models,
                                int B, int W, int max_steps, const comic_beam_constraints* constraints,
                                const comic_beam_groups* groups, const comic_beam_sampling* sampling,
                                const comic_beam_required* required, const int32_t* req, int32_t* step_ids,
                                int32_t* parent_ids, float* scores, int64_t* lengths, int32_t* finished,
                                float* const* attn_hists, int32_t* steps_executed, void* workspace, int64_t workspace_bytes,
                                void* stream);

/* Which decode a beam search is, as ONE value (extends rnn_decoder_beam_search, common/ops_rnn.py:49-112): the options of
 * the six entries above, each with the rules it has there.  Every pointer may be NULL: that option is off; a NULL record
 * is comic_decoder_beam_ensemble.  Refused before anything else is read: required words with more than one group or with
 * sampling, sampling with more than one group, a truncation without sampling, required words without their table.
 * comic_decoder_beam_search is the ONE executor loop and the entry the Python package calls; the named entries above are
 * its stable per-option forms: their own null checks and one forwarding call.  The workspace depends on which options are
 * present only (and, under constraints or required words, on max_steps): comic_decoder_beam_search_workspace returns what
 * the named query of the same combination returns, -1 where that does. */
typedef struct comic_beam_options {
  const comic_beam_constraints* constraints;
  const comic_beam_groups* groups;
  const comic_beam_sampling* sampling;
  const comic_beam_truncation* truncation; /* needs sampling */
  const comic_beam_required* required;     /* needs req; not with groups > 1 or sampling */
  const int32_t* req;                      /* device [B][n_words][stride] */
} comic_beam_options;
int64_t comic_decoder_beam_search_workspace(const comic_decoder_desc* descs, int n_models, int rows, int max_steps,
                                            const comic_beam_options* options);
int comic_decoder_beam_search(const comic_decoder_desc* descs, const comic_decoder_params* params, const float* const* fms,
                              const float* const* im_embeds, const float* weights, int n_models, int B, int W,
                              int max_steps, const comic_beam_options* options, int32_t* step_ids, int32_t* parent_ids,
                              float* scores, int64_t* lengths, int32_t* finished, float* const* attn_hists,
                              int32_t* steps_executed, void* workspace, int64_t workspace_bytes, void* stream);

/* Forced-prefix decoding (extends rnn_decoder_beam_search, common/ops_rnn.py:49-112): every caption of image b starts
 * with the tokens of row b of pfx, device int32 [B][max_tokens], padded with -1 at the end of each row (the length is the
 * index of the first -1; it may be 0 and differs per image).  At step t row (b, w) is FORCED when t < max_tokens,
 * 0 <= pfx[b][t] < V and the row is live: it may emit pfx[b][t] alone -- its ban mask has every bit below V set except
 * that token's, REPLACING what the constraints put there (inside the prefix the prefix wins over min_length, n-gram
 * blocking and suppressed words).  A row that is not forced keeps the constraints' mask, or an all-zero one; a finished
 * row bans nothing.  The mask is applied after the log-softmax: the forced token keeps the model's own step
 * log-probability, and log_probs / scores are the model's log p(prefix + continuation | image).  Lengths, the length
 * penalty, min_length, the n-gram histories and the required-word bookkeeping count the forced tokens; a required word
 * the prefix contains counts as produced.
 * A forced live row has ONE finite candidate, so the steps' precondition "every live beam keeps W unbanned candidates"
 * holds from step len on, not inside the prefix.  There the other slots follow the steps' all-(-inf) rule: plain beam
 * and each group: the first slot carries the prefix, the others hold totals of -inf and lose to the carrier's candidates
 * at the first free step; samples: every slot is a chain of its own and carries it; banks: the candidate lands in the bank
 * its progress selects, the other slots are dead slots.  No -inf slot is an ancestor of a slot with a finite final score.
 * The record travels beside comic_beam_options, not in it (that record is frozen). */
typedef struct comic_beam_prefix {
  int32_t max_tokens;                      /* P, the width of the table: 1 <= P < max_steps */
} comic_beam_prefix;
/* The masks of step t as a raw operator (common/ops_rnn.py:49-112; csrc/beam_prefix.hip): one launch for all B*W rows.
 * pfx [B][P], finished [B*W], bits [B*W][ceil(V/32)] (16-byte aligned).  has_bans as for comic_beam_truncate: != 0: bits
 * holds the constraints' mask (comic_beam_bans) and is updated in place (forced and finished rows are rewritten, the
 * others untouched); 0: every word of every row is written.  t >= P forces nobody.  A table entry outside [0,V) is "not
 * forced", never an index.  V <= 65 536. */
int comic_beam_prefix_mask(const int32_t* pfx, const int32_t* finished, uint32_t* bits, int t, int B, int W, int V, int P,
                           int has_bans, void* stream);
/* comic_decoder_beam_search (common/ops_rnn.py:49-112) from a prefix.  options may be NULL.  prefix NULL: exactly
 * comic_decoder_beam_search / its workspace query (which are these calls with a NULL prefix); else pfx must not be NULL,
 * 1 <= max_tokens < max_steps and V <= 65 536, checked before anything is read.  For t < max_tokens every step writes
 * the masks (after comic_beam_bans, before comic_beam_truncate and comic_beam_required_table) and ranks through them
 * whichever policy is on; for t >= max_tokens the launches are those of the same decode without a prefix.  max_tokens is
 * baked into a captured graph; the table's content is read at run time. */
int64_t comic_decoder_beam_search_prefixed_workspace(const comic_decoder_desc* descs, int n_models, int rows, int max_steps,
                                                     const comic_beam_options* options, const comic_beam_prefix* prefix);
int comic_decoder_beam_search_prefixed(const comic_decoder_desc* descs, const comic_decoder_params* params,
                                       const float* const* fms, const float* const* im_embeds, const float* weights,
                                       int n_models, int B, int W, int max_steps, const comic_beam_options* options,
                                       const comic_beam_prefix* prefix, const int32_t* pfx, int32_t* step_ids,
                                       int32_t* parent_ids, float* scores, int64_t* lengths, int32_t* finished,
                                       float* const* attn_hists, int32_t* steps_executed, void* workspace,
                                       int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* Op-level entries of the executor-only kernel forms                        */
/* ------------------------------------------------------------------------- */
/* The public ops above reach the decoder kernels with every executor-only argument null, 0 or 1.  The executors
 * (training, greedy / beam decode, sampling, scoring) launch the forms below; each entry forwards its arguments to the
 * internal entry the executors call and does nothing else, so one form can be compared with a reference on its own
 * operands.  No product code calls them; the arguments are those of the kernels (csrc/decoder.hip, csrc/cells.hip,
 * csrc/gemm.hip), in short:
 *   comic_attn_splits(B, M)      workgroups per batch row of the split attention forms (1: one-workgroup form);
 *   comic_attn_bwd_scratch       floats behind ws_d for the split backward (d alpha_d [B][H][M] + the partial rows);
 *   comic_op_attn_fwd            lens/t/att_prev -> att_next = finished ? att_prev : ctx; xh_next[b*xh_ld + c] =
 *                                drop(att_next) under mask_next / keep_in; q_parts > 1: q is [q_parts][B][D] split-K
 *                                partials, summed in slice order (also to q_out); scores_ws ([B][H][M] floats) enables
 *                                the split form when comic_attn_splits > 1; mem_div = W > 1: keys / values are held once
 *                                per B / W entries;
 *   comic_op_attn_bwd            pgrad_overwrite 0 adds this step's parameter-gradient row, 1 stores it, 2 is the split
 *                                form (dq and the pgrad rows zero-filled by the caller; softmax only): two workgroups
 *                                per row, or with ws_s ([B][H][M]) and ws_d (comic_attn_bwd_scratch floats) and
 *                                comic_attn_splits > 2 the partial-rows form with a fixed-order reduce;
 *   comic_op_xent / _maploss     t_rows <= t_stride time steps; d logits rows of ld_dl >= V floats (padding zeroed); the
 *                                map loss mean((1 - sum_h hist)^2) * scale with its gradient dmap (may be NULL) in the
 *                                same launch; partial: ceil(t_rows*B*M / 256) floats; *ticket zero before and after;
 *   comic_op_lstm_gates_*        g is [S][B][4D] split-K partials + bias; dy_part [S][B][D]; xh_next row stride xh_ld;
 *   comic_op_colsum_ws           two-stage column sum from 256 rows on (ws: 64*cols floats; NULL: comic_colsum);
 *   comic_gemm_f32_partial       ws receives [*S_out][M][N] raw split-K partial products of A[M,K] * op(B);
 *   comic_cell_ln_stride(D)      floats between the ten LayerNorm vectors of comic_decoder_params::cell_ln;
 *   comic_op_ln_lstm_* / _gru_*  the element-wise / row-wise halves of an LN_LSTM / GRU step (csrc/cells.hip). */
int comic_attn_splits(int B, int M);
long comic_attn_bwd_scratch(int B, int H, int M, int D);
int comic_cell_ln_stride(int D);
int comic_gemm_f32_partial(const float* A, const float* B, int M, int N, int K, int lda, int ldb, int trans_b, void* ws,
                           int64_t ws_bytes, int* S_out, void* stream);
int comic_op_attn_fwd(const comic_attn_desc* d, const float* keys, const float* values, const float* q, const float* ln_g,
                      const float* ln_b, const float* v, const float* tau, const float* mask_alpha, float keep_alpha,
                      float* alpha, float* alpha_d, float* ctx, const int32_t* lens, int t, const float* att_prev,
                      float* att_next, float* xh_next, int xh_ld, const float* mask_next, int mask_ld, float keep_in,
                      int q_parts, float* q_out, float* scores_ws, int mem_div, void* stream);
int comic_op_attn_bwd(const comic_attn_desc* d, const float* keys, const float* values, const float* q, const float* ln_g,
                      const float* ln_b, const float* v, const float* tau, const float* alpha, const float* mask_alpha,
                      float keep_alpha, const float* dctx, const float* dmap, float* dq, float* dkeys, float* dvalues,
                      float* pgrad, const int32_t* lens, int t, int pgrad_overwrite, float* ws_s, float* ws_d,
                      void* stream);
int comic_op_xent(float* logits, const int32_t* targets_bt, const float* coef_bt, const float* wmask_bt,
                  const int32_t* lens, float* loss_rows, float* dlogits, int32_t* ids_tb, int t_rows, int t_stride, int B,
                  int V, void* stream);
int comic_op_xent_maploss(float* logits, const int32_t* targets_bt, const float* coef_bt, const float* wmask_bt,
                          const int32_t* lens, float* loss_rows, float* dlogits, int ld_dl, int32_t* ids_tb, int t_rows,
                          int t_stride, int B, int V, const float* hist, float* dmap, float* partial, float* map_loss,
                          uint32_t* ticket, int H, int M, float scale, void* stream);
int comic_op_lstm_gates_fwd(const float* g, const float* c_prev, const float* h_prev, float* gates_act, float* c_new,
                            float* y, const float* mask_out, float keep_out, const int32_t* lens, int t, float* c_state,
                            float* h_state, int B, int D, float* xh_next, int xh_ld, int S, const float* bias,
                            void* stream);
int comic_op_lstm_gates_bwd(const float* gates_act, const float* c_prev, const float* c_new, const float* dy,
                            const float* dy_part, int S, const float* mask_out, float keep_out, const int32_t* lens, int t,
                            float* dc_state, float* dh_state, float* dg, int B, int D, void* stream);
int comic_op_colsum_ws(const float* in, float* out, int rows, int cols, float beta, float* ws, void* stream);
int comic_op_ln_lstm_fwd(const float* g, int S, const float* ln, const float* c_prev, const float* h_prev,
                         float* gates_act, float* xhat, float* rstd, float* c_new, float* y, const float* mask_out,
                         float keep_out, const int32_t* lens, int t, float* c_state, float* h_state, int B, int D,
                         float* xh_next, int xh_ld, void* stream);
int comic_op_ln_lstm_bwd(const float* gates_act, const float* xhat, const float* rstd, const float* ln,
                         const float* c_prev, const float* c_new, const float* dy, const float* dy_part, int S,
                         const float* mask_out, float keep_out, const int32_t* lens, int t, float* dc, float* dh, float* dg,
                         float* pgrad, int B, int D, void* stream);
int comic_op_ln_lstm_scatter(const float* sums, float* cell_ln_grad, int D, float beta, void* stream);
int comic_op_gru_gates_fwd(const float* g1, int S, const float* bias, const float* h_prev, const float* xh, int xh_ld,
                           float* ru, int ld_ru, float* xh2, int xh2_ld, int B, int D, int EA, void* stream);
int comic_op_gru_out_fwd(const float* g2, int S, const float* bias, const float* ru, int ld_ru, const float* h_prev,
                         float* cand, int ld_cand, float* y, const float* mask_out, float keep_out, const int32_t* lens,
                         int t, float* h_state, float* xh_next, int xh_ld, int B, int D, void* stream);
int comic_op_gru_bwd1(const float* dy, const float* dy_part, int S, const float* mask_out, float keep_out,
                      const int32_t* lens, int t, float* dh_state, const float* ru, int ld_ru, const float* cand,
                      int ld_cand, const float* h_prev, float* dpre, int ld_dpre, int B, int D, void* stream);
int comic_op_gru_bwd2(float* dxh2, int ld, const float* ru, int ld_ru, const float* h_prev, float* dpre, int ld_dpre, int B,
                      int D, int EA, void* stream);
/* The fused and streaming LSTM step kernels (csrc/decoder_fused.hip, csrc/lstm_stream.hip, csrc/lstm_prep.h) and the operand
 * hand-off behind the beam merge (csrc/beam_logits.hip).  The first three take the RAW row-major parameter and a panel
 * scratch, pack it as the executors do once per call, and launch the per-step host function:
 *   comic_op_lstm_step_fused     K [Wd][4D]; panel_floats >= ceil(D/4) * ceil(Wd/16) * 256; xh rows of ld_xh floats, xh_next
 *                                rows of xh_ld floats (only D columns written); stop (may be NULL): a device word, the
 *                                launches write nothing when *stop <= stop_t (the decode loops' early exit);
 *   comic_op_input_grad_fused    K [Wd][4D]; panel_floats >= ceil(Wd/16) * (4D/16) * 256; demb may be NULL; datt is read and
 *                                written ((carry && !finished ? 0 : old) + v), dh accumulated;
 *   comic_op_lstm_grad_fused     W_q [D][D]; panel_floats >= D*D; D % 16 == 0, an error otherwise (nothing written);
 *   comic_op_infer_lstm_step     the LSTM half of a decode step: row r gathers att / h / c of source row
 *                                (r / W) * W + clamp(parent[r], 0, W - 1) (parent NULL: r), an id outside [0, V) embeds as
 *                                zeros; stream_lstm = 0: the fp32 gather + the fused step (x_frag / y_frag unused);
 *                                1: the streaming step (33 ... 256 rows, D % 16 == 0, E % 8 == 0, A % 8 == 0, an error
 *                                otherwise), which also leaves the operand rows and y as bf16 hi / lo fragments
 *                                [16-row tile][k32-step][hi, lo][lane (r % 16, seg % 4)] x 8 bf16: ceil16(R) * ceil(Wd/32) * 32
 *                                and ceil16(R) * ceil(D/32) * 32 floats;
 *   comic_op_beam_step_prep      comic_beam_step_dense (same workspace) that also prepares the NEXT step's operand rows
 *                                (x_frag as above, c_in [B W][D]) through the words and parents it has just chosen; an
 *                                error where neither the merge kernel (V >= 4096, D % 128 == 0) nor the small step
 *                                (V <= 1024, W <= 8) serves the shape. */
int comic_op_lstm_step_fused(const float* K, float* panel, int64_t panel_floats, const float* xh, int ld_xh,
                             const float* bias, const float* c_prev, const float* h_prev, float* gates_act, float* c_new,
                             float* y, const float* mask_out, float keep_out, const int32_t* lens, int t, float* c_state,
                             float* h_state, float* xh_next, int xh_ld, int B, int D, int Wd, const int32_t* stop,
                             int stop_t, void* stream);
int comic_op_input_grad_fused(const float* K, float* panel, int64_t panel_floats, const float* dg, const float* mask,
                              float keep, float* demb, float* datt, float* dh, const int32_t* lens, int t, int carry, int B,
                              int E, int A, int D, void* stream);
int comic_op_lstm_grad_fused(const float* W_q, float* panel, int64_t panel_floats, const float* dq, const float* gates_act,
                             const float* c_prev, const float* c_new, const float* dy, const float* mask_out,
                             float keep_out, const int32_t* lens, int t, float* dc_state, float* dh_state, float* dg, int B,
                             int D, void* stream);
int64_t comic_op_infer_lstm_step_workspace(int R, int D, int E, int A, int stream_lstm);
int comic_op_infer_lstm_step(const float* table, const int32_t* ids, const int32_t* parent, int W, const float* att_src,
                             const float* h_src, const float* c_src, const float* K, const float* bias, float* c_in,
                             float* c2, float* h2, float* y, void* x_frag, void* y_frag, int R, int E, int A, int D, int V,
                             int stream_lstm, const int32_t* stop, int stop_t, void* workspace, int64_t workspace_bytes,
                             void* stream);
int comic_op_beam_step_prep(const float* y, const float* W_o, const float* b_o, float* log_probs, int32_t* finished,
                            int64_t* lengths, int32_t* word_ids, int32_t* parent_ids, float* scores, int B, int W, int D,
                            int V, int end_id, const float* table, const float* att, const float* h, const float* c,
                            void* x_frag, float* c_in, int E, int A, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* SCST reward scorer (host, multi-threaded)  common/scst/scorers.py:43-171      */
/* ------------------------------------------------------------------------- */
typedef struct comic_scorer comic_scorer;
/* df entries: `ngrams_host` = n_entries NUL-terminated strings (words joined by ' '),
 * concatenated; counts_host[n_entries]; ref_len = number of images in the df corpus. */
comic_scorer* comic_scorer_create(const char* ngrams_host, const double* counts_host,
                                  int64_t n_entries, double ref_len);
void comic_scorer_destroy(comic_scorer* s);
/* hypos: n strings; refs: for hypothesis i, refs_per[i] strings, concatenated in order.
 * out_cider[n]; out_bleu[n*4] (BLEU-1..4 per sentence, 'closest' reflen). */
int comic_scorer_score(const comic_scorer* s, const char* const* hypos_host, int n,
                       const char* const* refs_host, const int32_t* refs_per_host,
                       double* out_cider_host, double* out_bleu_host, int n_threads);

/* CRC-32C of a host buffer, continuing from `crc` (0 to start): checksum of the TF checkpoint-V2
 * container the reference's tf.train.Saver reads and writes (train_fn.py:67-70,131-132). */
uint32_t comic_crc32c(const void* data_host, size_t n, uint32_t crc);

#ifdef __cplusplus
}
#endif
#endif /* COMIC_HIP_H_ */
