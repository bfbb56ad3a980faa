/* bsmi.h -- C ABI of libbsmi.so, the MI355X (gfx950) engine behind the
 * `bs predict` / `bs segment --ws` hot path of ucsdmanorlab/bootstrapper.
 *
 * Plain pointers and sizes only; no torch / numpy types.  All functions return
 * 0 on success and a negative code on failure; the message for the calling
 * thread is available from bsmi_last_error().  No exception crosses this
 * boundary.  Pointers suffixed _dev are device (HBM) pointers on the handle's
 * device, _host are host pointers.  `stream` is a hipStream_t passed as void*
 * (NULL = the null stream); calls are asynchronous on it unless stated.
 *
 * Every entry point names the reference interface it replaces (paths relative
 * to /root/reference/bootstrapper).
 */
#ifndef BSMI_H
#define BSMI_H

#include <stddef.h>
#include <stdint.h>
#include <sys/types.h> /* ssize_t */

#ifdef __cplusplus
extern "C" {
#endif

#define BSMI_MAX_LEVELS 8
#define BSMI_MAX_CONVS 4
#define BSMI_MAX_HEADS 4
#define BSMI_NAME_LEN 32

#define BSMI_OK 0
#define BSMI_ERR_INVALID (-1)   /* bad argument / shape the network cannot take */
#define BSMI_ERR_HIP (-2)       /* HIP runtime error                            */
#define BSMI_ERR_STATE (-3)     /* call order (e.g. forward before finalize)    */
#define BSMI_ERR_MISSING (-4)   /* missing / unexpected state-dict key          */
#define BSMI_ERR_OVERFLOW (-5)  /* a fixed-capacity device structure overflowed */

/* arithmetic type of the U-Net contraction */
#define BSMI_PREC_F32 0   /* f32 MFMA (exact f32 products, f32 accumulate): parity mode */
#define BSMI_PREC_BF16 1  /* bf16 MFMA operands, f32 accumulate: throughput mode        */
#define BSMI_PREC_BF16X3 2 /* split bf16: every f32 operand x = hi + lo (two bf16), products hi*hi + lo*hi + hi*lo
                              on the bf16 MFMA, f32 accumulate; activations stored as (hi, lo) planes.  Within the
                              1e-4 parity gate of the fp32 reference at 3 MFMAs per product                        */
#define BSMI_NUM_PREC 3

/* dtype of the raw input handed to bsmi_unet_forward */
#define BSMI_RAW_U8 0     /* uint8 [Cin][D][H][W]; normalised on device as u8/255*2-1    */
#define BSMI_RAW_F32 1    /* float [Cin][D][H][W]; already normalised                    */
#define BSMI_RAW_U8_UNIT 2 /* uint8 [Cin][D][H][W]; normalised on device as u8/255: predictions
                              fed to a second-stage net (models/3d_affs_from_2d_mtlsd/predict.py:163-164) */

const char *bsmi_last_error(void);
int bsmi_version(void);

/* ------------------------------------------------------------------------ */
/* 3-D U-Net (reference: models/3d_affs/unet.py:226-478 UNet, :7-76 ConvPass,
 * :79-106 Downsample, :109-223 Upsample; models/3d_affs/model.py:28-64 Model;
 * models/3d_mtlsd/model.py:28-68).                                            */

/* Mirrors the keys of net_config.json that Model() consumes
 * (models/3d_affs/model.py:10-25, net_config.json) plus the head list the
 * Model class hard-codes (model.py:54-56; mtlsd model.py:54-59).             */
typedef struct bsmi_unet_config {
  int32_t in_channels;
  int32_t num_fmaps;
  int32_t fmap_inc_factor;
  int32_t num_levels; /* len(downsample_factors) + 1 */
  int32_t downsample_factors[BSMI_MAX_LEVELS][3];
  int32_t n_convs_down[BSMI_MAX_LEVELS];
  int32_t kernel_size_down[BSMI_MAX_LEVELS][BSMI_MAX_CONVS][3];
  int32_t n_convs_up[BSMI_MAX_LEVELS];
  int32_t kernel_size_up[BSMI_MAX_LEVELS][BSMI_MAX_CONVS][3];
  int32_t num_heads;
  char head_name[BSMI_MAX_HEADS][BSMI_NAME_LEN]; /* state-dict prefix, forward() return order */
  int32_t head_dims[BSMI_MAX_HEADS];
  int32_t num_fmaps_out; /* channels of the last right-side ConvPass (unet.py:239,344,426); 0 = num_fmaps.
                            Set by the second-stage nets (net_config.json of the models/3d_affs_from_... setups) */
} bsmi_unet_config;

typedef struct bsmi_unet bsmi_unet;

/* replaces Model.__init__ (model.py:30-56) on `device` */
int bsmi_unet_create(const bsmi_unet_config *cfg, int device, bsmi_unet **out);
int bsmi_unet_destroy(bsmi_unet *h);

/* replaces Model.load_state_dict (models/3d_affs/predict.py:103-107): one call per
 * state-dict entry, `key` WITHOUT the Lightning "model." prefix, data OIDHW fp32. */
int bsmi_unet_load_weight(bsmi_unet *h, const char *key, const float *data_host,
                          const int64_t *shape, int ndim);
/* strict check (every expected key loaded) + pack/upload weights for `precision`;
 * may be called once per precision. */
int bsmi_unet_finalize(bsmi_unet *h, int precision);

/* valid-conv shape arithmetic (unet.py:96-104 divisibility, :147-201 crop_to_factor) */
int bsmi_unet_output_shape(bsmi_unet *h, const int64_t in_shape[3], int64_t out_shape[3]);
/* algorithmic multiply-add count x2 for one forward at in_shape (SURVEY 8a table:
 * residual 1x1x1 counted on the cropped extent) */
int bsmi_unet_flops(bsmi_unet *h, const int64_t in_shape[3], double *flops);

/* replaces Model.forward (model.py:58-64) + the predict worker's arithmetic around
 * it (models/3d_affs/predict.py:145-154): raw -> heads.  For each head i either
 * output pointer may be NULL:
 *   out_f32_dev[i]: float  [head_dims[i]][d][h][w]  sigmoid outputs
 *   out_u8_dev[i] : uint8  [head_dims[i]][d][h][w]  (uint8)(sigmoid*255), truncation
 * Device workspace for the given in_shape is allocated on first use and cached. */
int bsmi_unet_forward(bsmi_unet *h, int precision, const void *raw_dev, int raw_dtype,
                      const int64_t in_shape[3], float *const *out_f32_dev,
                      uint8_t *const *out_u8_dev, void *stream);

/* ---- training (reference models/3d_affs/train.py:152-159, model.py:67-92; fp32 like the reference) ------------
 * begin: after bsmi_unet_finalize(h, BSMI_PREC_F32); builds the backward plan for in_shape and moves the
 *   parameters into a flat fp32 device buffer (sorted state_dict keys, each padded to 4 floats).
 * forward_backward: raw_dev float32 [Cin][D][H][W] (already normalised, as the training pipeline delivers it);
 *   targets_dev[i] / weights_dev[i]: float32 [head_dims[i]][d][h][w] per head, in Model.forward order; the loss is
 *   the sum over heads of WeightedMSELoss; gradients of all parameters land in the flat gradient buffer
 *   (zeroed first).  loss_host (optional) synchronises the stream.
 * buffers: the flat parameter / gradient device buffers (the gradient buffer is what data-parallel training
 *   all-reduces); param_info: offset and count of one state_dict key inside them.
 * adam_step: torch.optim.Adam semantics (no weight decay); grad_scale multiplies the gradients first (1/world_size
 *   after a summing all-reduce); the packed weight images of all launches are rewritten from the new parameters.
 * read_param: what = 0 parameter, 1 gradient, 2 / 3 Adam moments -> host.  end: frees the training state; the trained
 *   parameters stay the handle's weights (re-finalize BSMI_PREC_BF16 before predicting in bf16).
 * set_arithmetic (before begin): 1 (default) = the convolutions of the step -- forward, input gradients, weight gradients --
 *   multiply as split-bf16 (every f32 operand = bf16 hi + bf16 lo, hi*hi + lo*hi + hi*lo accumulated in f32: 2^-17
 *   relative per product, what BSMI_PREC_BF16X3 is to inference) while every tensor, the loss, the gradient buffer and
 *   Adam stay fp32; 0 = exact f32 MFMA throughout (half the speed). */
int bsmi_unet_train_set_arithmetic(bsmi_unet *h, int split_bf16);
/* set_deterministic (any time; default 0): 1 = every reduction of the step that float atomics would order by chance -- the loss
 *   sums, the head's and the biases' gradients, the weight gradients of launches cut into line ranges, the transposed
 *   interpolation -- is done as per-workgroup partial results added in index order: two runs of a step on the same inputs give
 *   the same bits (gradients, loss, parameters after Adam), like the reference's CPU path.  Costs about an eighth of the step
 *   (21.2 against 18.7 ms on the (32,196,196) block). */
int bsmi_unet_train_set_deterministic(bsmi_unet *h, int on);
int bsmi_unet_train_begin(bsmi_unet *h, const int64_t in_shape[3]);
int bsmi_unet_train_forward_backward(bsmi_unet *h, const float *raw_dev, const float *const *targets_dev,
                                     const float *const *weights_dev, float *loss_host, void *stream);
int bsmi_unet_train_num_params(bsmi_unet *h, uint64_t *count);
int bsmi_unet_train_buffers(bsmi_unet *h, float **params_dev, float **grads_dev);
int bsmi_unet_train_param_info(bsmi_unet *h, const char *key, uint64_t *offset, uint64_t *count);
int bsmi_unet_train_adam_step(bsmi_unet *h, float lr, float beta1, float beta2, float eps, float grad_scale,
                              void *stream);
int bsmi_unet_train_read_param(bsmi_unet *h, const char *key, int what, float *host_out);
/* last_loss: the loss of the last forward_backward (synchronises `stream`), for callers that passed loss_host = NULL to
 *   keep the step asynchronous.
 * grad_groups: the flat buffers cut into the ranges whose gradients become final together (one per ConvPass / head), in
 *   the order the backward pass finishes them; wait_grad_group makes `stream` wait until the last forward_backward has
 *   finished group g -- a data-parallel caller reduces group after group on a side stream while the backward pass
 *   still runs (the implicit DDP of training.py:125-133 overlaps bucket all-reduces the same way).
 * write_param (what = 2 / 3) and step_count restore the Adam moments and step of a checkpoint (Lightning resumes them,
 *   training.py:131-137 ckpt_path); step_count(set_to < 0) only reads. */
int bsmi_unet_train_last_loss(bsmi_unet *h, float *loss_host, void *stream);
/* the sigmoid outputs of head `head` from the last forward_backward, float [dims][d][h][w] on the device (what the
 * reference's training_step returns as pred_<head> for the snapshot callback, models/3d_mtlsd/train.py:183-187) */
int bsmi_unet_train_prediction(bsmi_unet *h, int head, float **out_dev, uint64_t *count);
int bsmi_unet_train_grad_groups(bsmi_unet *h, int max_n, int *n, uint64_t *offsets, uint64_t *counts);
int bsmi_unet_train_wait_grad_group(bsmi_unet *h, int group, void *stream);
int bsmi_unet_train_write_param(bsmi_unet *h, const char *key, int what, const float *host_in);
int bsmi_unet_train_step_count(bsmi_unet *h, int set_to, int *value);
int bsmi_unet_train_end(bsmi_unet *h);

/* Development aid (read-only): a gradient tensor of plan step `step` (numbering of bsmi_unet_debug_step_info) as the last
 * bsmi_unet_train_forward_backward left it, float32 channels-last [D][H][W][C] on the host, real channels only.  Every such
 * tensor is allocated once in bsmi_unet_train_begin and stays resident, so this only copies; it synchronises the device
 * (the weight gradients' side stream included).  shape_out = {D, H, W, C}; host_out may be NULL to query the shape.
 * A step that has no such tensor fails with BSMI_ERR_STATE. */
enum {
  BSMI_TRAIN_DBG_DOUT = 0,      /* dL/d(output of the step); conv, pool and up steps, and the net's input where it has one */
  BSMI_TRAIN_DBG_GMASK = 1,     /* conv: the padded masked gradient dY [Y > 0], whole, zero border included */
  BSMI_TRAIN_DBG_GSPLIT = 2,    /* conv: its split-bf16 copy as hi + lo (where the input gradient is a split launch) */
  BSMI_TRAIN_DBG_GSPLIT_HI = 3, /* ... the hi plane */
  BSMI_TRAIN_DBG_GSPLIT_LO = 4, /* ... the lo plane */
  BSMI_TRAIN_DBG_DCAT = 5,      /* conv 0 of a ConvPass: the gradient of its (cropped, concatenated) input before the scatter */
  BSMI_TRAIN_DBG_HEAD_DP = 6,   /* head: dL/dp */
  BSMI_TRAIN_DBG_PAD_COUNT = 7  /* conv: shape {1, 1, 1, 4}: the number of non-zero values the kernels read as zeros -- in the
                                 * padding channels (C .. Cpad) of the masked gradient, in its border (all channels), in the
                                 * padding channels of the output gradient, and of the concat-input gradient (0 without one) */
};
int bsmi_unet_train_debug_tensor(bsmi_unet *h, int step, int what, int64_t shape_out[4], float *host_out,
                                 uint64_t capacity);

/* What the last backward pass ran for plan step `step`, recorded where each launch was issued. */
enum { BSMI_WGRAD_NONE = 0, BSMI_WGRAD_WAVE_F32 = 1, BSMI_WGRAD_TILED_F32 = 2, BSMI_WGRAD_SPLIT = 3 };
typedef struct {
  int32_t family;          /* BSMI_WGRAD_* */
  int32_t residual;        /* 1: a slot of the cropped 1x1x1 residual branch */
  int32_t n, c, cbase;     /* real output / input channels of the slot, its first column in the weight */
  int32_t kx;              /* x taps one workgroup accumulates */
  int32_t tile_n, tile_c;  /* (n, c) block of one workgroup */
  int32_t ranges, lines_per_range;  /* line ranges the launch was cut into, output lines (z, y) in each */
  int32_t det_workspace;   /* 1: every range added into its own copy of the workspace (deterministic mode) */
} bsmi_unet_train_wgrad_info;
typedef struct {
  int32_t type;            /* BSMI_STEP_* */
  int32_t n_wgrad;         /* conv: weight-gradient launches, main slots first, then the residual's */
  bsmi_unet_train_wgrad_info wgrad[4];
  int32_t dgrad;           /* conv: input gradient 0 none, 1 exact f32, 2 split-bf16 */
  int32_t dgrad_raw;       /* split: the launch stored raw f32 sums */
  int32_t dgrad_converted; /* split: (hi, lo) pairs, then split_to_f32_kernel */
  int32_t dgrad_bn, dgrad_ksteps, dgrad_split_k, dgrad_scatter, dgrad_residual;
  int32_t border[3];       /* conv: border of the padded masked gradient */
  int32_t has_split;       /* conv: a split copy of the masked gradient exists */
  int32_t bias;            /* conv: bias sums 0 none, 1 fused into the masking pass, 2 colsum_kernel */
  int32_t up;              /* up: 0 none, 1 scatter (float atomics), 2 gather */
  int32_t fwd_split;       /* conv: the training forward ran this step as a fused split-bf16 launch */
  int32_t deterministic;
} bsmi_unet_train_step_info;
int bsmi_unet_train_debug_step_info(bsmi_unet *h, int step, bsmi_unet_train_step_info *info);

/* Affinity training targets of one sample, on the device (reference models/3d_affs/train.py:127-139:
 * gp.GrowBoundary(labels, mask=unlabelled, steps, only_xy) -> gp.AddAffinities(neighborhood) ->
 * gp.BalanceLabels; the erosion as in gp/custom_grow_boundary.py:71-110 with a fixed step count).
 *   labels_dev      int64 [D][H][W], 0 = background; overwritten with the grown-boundary labels
 *   unlabelled_dev  uint8 [D][H][W] or NULL: 1 where the ground truth is known (CreateMask), 0 = unknown
 *   neighborhood    n offsets (z, y, x), host pointer (net_config "neighborhood")
 *   grow_steps      voxels of boundary to grow (net_config "grow_boundary"); a voxel keeps its label when every
 *                   voxel within that L1 distance (in its section if only_xy) has the same label, is unknown, or
 *                   lies outside the block (binary_erosion(iterations=steps, border_value=1))
 *   affs_dev        float [n][D][H][W]: 1 where p and p + offset carry the same non-zero label
 *   weights_dev     float [n][D][H][W]: affinity mask (both voxels inside the block, p known) scaled by
 *                   1 / (2 f) for positives and 1 / (2 (1 - f)) for negatives, f = masked positive fraction
 *                   clipped to [clip_min, clip_max] (BalanceLabels, slab = whole sample)                       */
int bsmi_train_affinity_targets(int device, int64_t *labels_dev, const uint8_t *unlabelled_dev,
                                const int64_t shape[3], const int32_t *neighborhood, int n, int grow_steps,
                                int only_xy, float clip_min, float clip_max, float *affs_dev,
                                float *weights_dev, void *stream);

/* Local-shape-descriptor training targets of one sample, on the device (reference models/3d_mtlsd/train.py:134-141:
 * AddLocalShapeDescriptor(labels, gt_lsds, unlabelled, lsds_mask, sigma, downsample) of the lsd package [EXT]; restated
 * in oracle/lsd_ref.py).  3-D descriptors, 10 channels: mean offset (z, y, x), variances, Pearson coefficients
 * (zy, zx, yx), size -- each in [0, 1].
 *   labels_dev   int64 [D][H][W]: the label crop grown by the window context (3 sigma; zeros where the volume ends)
 *   unlabelled_dev  uint8 [D][H][W] or NULL: 1 where the ground truth is known
 *   roi_offset / roi_shape  the output block inside that array (all multiples of `downsample`, like the lsd package asks)
 *   sigma, voxel_size  world units (net_config "sigma" is one number: the same for the three axes)
 *   lsds_dev     float [10][d][h][w];  weights_dev  float [10][d][h][w] or NULL: 1 on labelled, known voxels        */
int bsmi_train_lsd_targets(int device, const int64_t *labels_dev, const uint8_t *unlabelled_dev, const int64_t shape[3],
                           const int64_t roi_offset[3], const int64_t roi_shape[3], const float sigma[3],
                           const float voxel_size[3], int downsample, float *lsds_dev, float *weights_dev, void *stream);

/* 2-D local-shape-descriptor training targets of a batch of sections, in one launch (reference models/2d_mtlsd/train.py:
 * Add2DLSDs(labels, gt_lsds, unlabelled, lsds_mask, sigma=(0, s, s), downsample), gp/add_2d_lsds.py: lsd's LsdExtractor
 * [EXT] in 2-D on every section; restated in tests/lsd2d_ref.py).  6 channels: mean offset (y, x), variances (y, x), Pearson
 * yx, size -- each in [0, 1], 0 on background.  Statistics per (sub-grid cell, label), staged in LDS, f32.
 *   labels_dev   int64 [n_sections][H][W]: label sections grown by the window context (3 sigma; zeros where the volume ends)
 *   unlabelled_dev  uint8 [n_sections][H][W] or NULL: 1 where the ground truth is known
 *   roi_offset / roi_shape  the output window inside every section (all multiples of `downsample`)
 *   sigma, voxel_size  (y, x), world units; the window radius 3 sigma / (voxel_size * downsample) is at most 60
 *   lsds_dev     float [6][n_sections][h][w];  weights_dev  float [6][n_sections][h][w] or NULL: 1 on labelled, known voxels */
int bsmi_train_lsd2d_targets(int device, const int64_t *labels_dev, const uint8_t *unlabelled_dev, int n_sections,
                             const int64_t shape[2], const int64_t roi_offset[2], const int64_t roi_shape[2], const float sigma[2],
                             const float voxel_size[2], int downsample, float *lsds_dev, float *weights_dev, void *stream);

/* Affinity training targets of the output ROI of label arrays that carry the neighbourhood's context (gp.AddAffinities grows
 * its labels request by the neighbourhood; BalanceLabels then sees the output ROI only).  n_samples independent arrays:
 * GrowBoundary and the affinities on each whole array, the mask / balance as bsmi_train_affinity_targets states them,
 * with the positive fraction counted per sample over its ROI (the reference balances every draw before gp.Stack).
 *   labels_dev      int64 [n_samples][D][H][W]; overwritten with the grown-boundary labels
 *   unlabelled_dev  uint8 [n_samples][D][H][W] or NULL
 *   roi_offset / roi_shape  the output ROI inside every array
 *   affs_dev / weights_dev  float [n][n_samples][d][h][w] (for sections, D = d = 1: the (C, S, h, w) stack of a batch) */
int bsmi_train_affinity_targets_roi(int device, int64_t *labels_dev, const uint8_t *unlabelled_dev, int n_samples,
                                    const int64_t shape[3], const int64_t roi_offset[3], const int64_t roi_shape[3],
                                    const int32_t *neighborhood, int n, int grow_steps, int only_xy, float clip_min,
                                    float clip_max, float *affs_dev, float *weights_dev, void *stream);

/* Summed-area table of a stack of mask sections: sat_dev uint32 [n_sections][height + 1][width + 1],
 * sat[s][y][x] = number of non-zero mask voxels of section s above row y and left of column x.  The 2-D sample source
 * counts the known voxels of an output window with four lookups. */
int bsmi_train_mask_sat(int device, const uint8_t *mask_dev, int n_sections, int height, int width, uint32_t *sat_dev,
                        void *stream);

/* Number of CUs the stream bsmi_unet_forward is called on may use (a multiple of 8; -1 restores the
 * default = all CUs of the device, 0 disables the persistent launches).  The big-tile conv layers run
 * as that many persistent workgroups (conv_igemm.hip); set it when the stream carries a CU mask. */
int bsmi_unet_set_persistent_grid(bsmi_unet *h, int n_cus);

/* HIP stream restricted to the CUs of `cu_mask` (hipExtStreamCreateWithCUMask; on MI355X bit i selects a
 * CU of XCD i % 8, so the first 8k bits give k CUs in every XCD).  The block pipeline keeps its
 * latency-bound segmentation kernels and the U-Net on disjoint CU sets this way. */
int bsmi_stream_create_cu_mask(int device, const uint32_t *cu_mask, int n_words, void **stream_out);
int bsmi_stream_destroy(int device, void *stream);

/* Per-launch timing of the forward pass with HIP events recorded on the caller's stream
 * (bench.py's roofline leg).  on = N > 0: every Nth bsmi_unet_forward (N = 1: every one)
 * brackets each launch with events; on = 0 switches the timing off.
 * bsmi_unet_profile_read synchronises on them and returns, for the last timed forward, the launch type (0 input, 1 implicit-GEMM conv, 2 max-pool, 3 upsample+crop,
 * 4 head), its duration in ms and its algorithmic FLOPs. */
int bsmi_unet_profile_enable(bsmi_unet *h, int on);
int bsmi_unet_profile_read(bsmi_unet *h, int max_n, int *n, int32_t *types, double *ms,
                           double *flops);
/* totals over every profiled forward since the last reset, indexed by launch type */
int bsmi_unet_profile_totals(bsmi_unet *h, double ms_by_type[5], double flops_by_type[5],
                             int64_t launches_by_type[5], int reset);
/* FLOPs the matrix pipe was actually given by the profiled convolution launches since the last reset (tile padding, every
 * batch of a Winograd stage, three bf16 products per product of the split mode): the algorithmic count of
 * bsmi_unet_profile_totals says how fast the layer was computed, this one how busy the MFMA units were -- a Winograd stage
 * computes a layer with fewer multiplies than the algorithmic count has. */
int bsmi_unet_profile_executed(bsmi_unet *h, double *executed_flops, int reset);
/* Development aid: `blocks` one-wave workgroups that fill `lds_bytes` of LDS with a pattern, idle for `spins` x 127 x 64 clocks
 * and check it; *mismatches_dev (device uint64, caller-zeroed) counts words that changed.  Run beside an engine on another
 * stream: does a co-resident kernel write outside its own LDS allocation? */
int bsmi_debug_lds_canary(int lds_bytes, int blocks, int spins, unsigned long long *mismatches_dev, void *stream);
/* Development aid: with BSMI_GUARD_MB=<n> in the environment every device allocation of the network engine, the training state and
 * the segmentation engines lies between
 * two n-MiB zones of 0xFF bytes (csrc/dev_guard.h): a read past a buffer that reaches a result turns it into NaNs, and this
 * call counts the zones something WROTE into (0 = intact, each hit reported on stderr; -1 = HIP error; 0 when unset): those of
 * the live allocations plus those that checked releases (below, and the stream scratch of the training targets) have counted
 * since the last call. */
int bsmi_debug_check_guards(void);
/* The same guards around every tensor of torch's: the pair that torch.cuda.memory.CUDAPluggableAllocator(libbsmi.so, ...) takes
 * (`stream` is a hipStream_t).  malloc gives exactly `size` bytes between two zones, the far one beginning at byte `size`, on
 * `device` (the caller's device is restored); free waits for the device, reads that allocation's zones, reports each damaged one
 * on stderr ("torch tensor of N bytes"), adds them to the count of bsmi_debug_check_guards() and frees.  It never aborts, and
 * gives the check up quietly after a HIP error (interpreter shutdown).  Unset: plain hipMalloc / hipFree.
 * tests/test_redzones_gpu.py runs the parity tests of the kernels that work in the caller's tensors this way. */
void *bsmi_debug_torch_malloc(ssize_t size, int device, void *stream);
void bsmi_debug_torch_free(void *ptr, ssize_t size, void *stream);
/* Does the checker see what it must?  One guarded buffer of 1000 bytes; hipMemset writes single bytes into the buffer's own zones
 * (just past the end, just before the start, the outermost byte of each zone); the checker must name exactly those zones and
 * offsets, and a checked release must count them.  0 = it does; -1 = BSMI_GUARD_MB unset or a HIP error; > 0 = the failed step. */
int bsmi_debug_guard_selftest(void);

/* Development aid: the output tensor of launch `step` of the last forward (launch order as in
 * bsmi_unet_profile_read), as float32 channels-last [D][H][W][C] on the host, whatever the precision mode stores
 * (f32, bf16, or the hi + lo planes of the split mode).  shape_out = {D, H, W, C}; host_out may be NULL to query
 * the shape.  what: 0 = the value, 1 / 2 = only the hi / lo plane of the split mode.  Synchronises the device.
 * A step that the last forward did not materialise -- input preparation and the first convolution when the first ConvPass
 * ran as one launch, an upsampling step that was fused into its Winograd consumers -- fails with BSMI_ERR_STATE. */
int bsmi_unet_debug_activation(bsmi_unet *h, int step, int what, int64_t shape_out[4], float *host_out,
                               uint64_t capacity);

/* What launch `step` of the last forward's plan is (what BSMI_PLAN_DEBUG prints, as data). */
enum { BSMI_STEP_INPUT = 0, BSMI_STEP_CONV = 1, BSMI_STEP_POOL = 2, BSMI_STEP_UP = 3, BSMI_STEP_HEAD = 4 };
/* kernel form of a conv step */
enum {
  BSMI_FORM_GATHER = 0,        /* implicit GEMM, rows gathered per K-step (conv_igemm) */
  BSMI_FORM_RASTER_HALO = 1,   /* conv_rh */
  BSMI_FORM_BOX_HALO = 2,      /* conv_box */
  BSMI_FORM_HALO_RESIDENT = 3, /* conv_h16 */
  BSMI_FORM_FIRST_PASS = 4,    /* the whole first ConvPass as one launch (first_pass) */
  BSMI_FORM_WINO2 = 5,         /* Winograd F(2x2, 3x3) around the batched GEMM */
  BSMI_FORM_WINO4 = 6,         /* Winograd F(4x4, 3x3) */
  BSMI_FORM_COUNT = 7
};
/* flags of a conv step */
enum {
  BSMI_STEP_FUSED_UP = 1,      /* a source is read through an on-the-fly upsampling (the UP step before it is not materialised) */
  BSMI_STEP_RES_LOW = 2,       /* part of the residual branch runs as a GEMM of its own below the upsampling */
  BSMI_STEP_SPLIT_K = 4,       /* the launcher's rule sends (one of) the GEMM launches of this step to the persistent split-K form */
  BSMI_STEP_BELOW_UP = 8,      /* the 3x3x3 taps of the upsampled source run as nine (3,1,1) GEMM column groups below the upsampling */
  BSMI_STEP_WINO_Z = 16        /* Winograd F(4x4) stage that is F(2,3) along z as well: 144 batches over pairs of output planes */
};
typedef struct {
  int32_t type;          /* BSMI_STEP_* */
  int32_t materialised;  /* 0: the forward writes no tensor for this step; bsmi_unet_debug_activation refuses it */
  int32_t shape[4];      /* D, H, W, C of the step's output (head: of its input) */
  int32_t conv_index;    /* conv steps: index inside the ConvPass */
  int32_t form;          /* conv steps: BSMI_FORM_* */
  int32_t flags;         /* conv steps: BSMI_STEP_FUSED_UP | ... */
  int32_t bn;            /* conv steps: columns of the GEMM tile (0: the form has no such tile) */
  int32_t ksteps;        /* conv steps: K-steps of the (batched) GEMM as the kernel walks them */
  int32_t head;          /* head steps: index of the head */
  int32_t factor[3];     /* pool / up steps */
  int32_t offset[3];     /* up steps: crop origin inside the upsampled map */
  char prefix[64];       /* conv steps: state-dict prefix of the ConvPass; head steps: of the head */
} bsmi_unet_step_info;
/* *n_steps (optional) receives the number of steps; info may be NULL to query it alone. */
int bsmi_unet_debug_step_info(bsmi_unet *h, int step, bsmi_unet_step_info *info, int *n_steps);

/* Development aid, host only (no device is touched): the transformed weights of a Winograd F(4x4) stage as the host packs
 * them (the cross-check form of BSMI_WINO_PACK_HOST=1), for a stage whose V channels are its `cin` input channels padded to 16.
 * w: OIDHW f32 [cout][cin][3][3][3]; wz != 0: the form that is F(2,3) along z as well (144 batches, batch 36 e + b, K = channels
 * only), else 36 batches with the three z taps inside every 32-channel chunk.  The image is bf16 bit patterns, hi image then
 * lo image of image_elems values each: value (batch, K-step s, column n, element k of the 32) at
 * batch * batch_elems + (s * npad + n) * 32 + k.  out may be NULL to query the sizes; capacity in uint16 values. */
int bsmi_debug_wino_pack_host(const float *w, int cout, int cin, int wz, uint16_t *out, uint64_t capacity,
                              uint64_t *image_elems, uint64_t *batch_elems, int *npad, int *ksteps);

/* Reflect-padded block extraction (gp.Pad(raw, None, mode="reflect") +
 * ArraySource ROI read, models/3d_affs/predict.py:145-148): copies the window
 * [offset, offset+block_shape) of vol (uint8 [D][H][W]) into block, mirroring
 * coordinates outside the volume (numpy 'reflect': edge voxel not repeated). */
int bsmi_extract_block_reflect_u8(const uint8_t *vol_dev, const int64_t vol_shape[3],
                                  const int64_t offset[3], const int64_t block_shape[3],
                                  uint8_t *block_dev, void *stream);

/* ------------------------------------------------------------------------ */
/* Seeded watershed fragments (reference: post/ws.py:38-112
 * watershed_from_affinities, :8-35 watershed_from_boundary_distance).
 * affs_dev: uint8 [3][D][H][W] (z,y,x nearest-neighbour affinities).
 * frags_dev: uint64 [D][H][W].  max_id_dev: uint64[1] (ws.py return value n+id_offset).
 * Only fragments_in_xy != 0 and max_affinity_value = 255 are implemented.
 * bsmi_seg_create limits: 1 <= max_shape[d] <= 4096 on every axis (so sections up to 4096 x 4096: slices of 2^20 voxels and
 * more take the wide flood, whose spill the handle then allocates); fragment ids below 2^27.  The 3-D mode
 * (fragments_in_xy = 0) with the device flood (bsmi_seg_set_host_flood(h, 0)) takes volumes below 2^23 voxels with
 * D^2 + H^2 + W^2 + 2 D + 1 < 2^18; with the host flood (the default) volumes below 2^31 voxels (the device stages before
 * it index voxels in 32 bits).  A call's slice is bounded by the handle's H * W; a slice of 2^20 voxels or more must also
 * keep H, W <= 4096 (BSMI_ERR_INVALID otherwise).                                                                    */
typedef struct bsmi_seg bsmi_seg;
int bsmi_seg_create(int device, const int64_t max_shape[3], bsmi_seg **out);
int bsmi_seg_destroy(bsmi_seg *h);

int bsmi_ws_fragments_u8(bsmi_seg *h, const uint8_t *affs_dev, const int64_t shape[3],
                         int fragments_in_xy, int min_seed_distance, uint64_t *frags_dev,
                         uint64_t *max_id_dev, void *stream);

/* The same with `return_seeds` (ws.py:42,105-110): seeds_dev (uint64 [D][H][W], may be NULL) receives the labelled
 * maxima before they meet the mask, with the same id offsets as the fragments they grow into. */
int bsmi_ws_fragments_seeds_u8(bsmi_seg *h, const uint8_t *affs_dev, const int64_t shape[3],
                               int fragments_in_xy, int min_seed_distance, uint64_t *frags_dev,
                               uint64_t *max_id_dev, uint64_t *seeds_dev, void *stream);

/* Mean-affinity hierarchical agglomeration (reference call site
 * post/watershed.py:333-338 waterz.agglomerate(affs, thresholds, fragments,
 * "OneMinus<MeanAffinity<RegionGraphType, ScoreValue>>"); algorithm restated in
 * oracle/seg_ref.c).  For each threshold t (ascending) writes
 * segs_dev + t*D*H*W: uint64 [D][H][W].  frags_dev is not modified.               */
int bsmi_agglomerate_mean_u8(bsmi_seg *h, const uint8_t *affs_dev, const uint64_t *frags_dev,
                             const int64_t shape[3], const float *thresholds_host,
                             int n_thresholds, uint64_t *segs_dev, void *stream);

/* The same hierarchical agglomeration with a histogram-quantile scorer (reference post/watershed.py:230-243:
 * merge_function "hist_quant_<Q>[_initmax]" = "OneMinus<HistogramQuantileAffinity<RegionGraphType, Q, ScoreValue, 256,
 * init_with_max>>"; waterz call site post/watershed.py:333-338).  The region graph and the 256-bin histogram of every edge's
 * affinities are built on the device, the merge loop runs on the host (as waterz's does), the relabel on the device.
 * Synchronises the stream.  Outputs as bsmi_agglomerate_mean_u8.                                                     */
int bsmi_agglomerate_hist_u8(bsmi_seg *h, const uint8_t *affs_dev, const uint64_t *frags_dev,
                             const int64_t shape[3], const float *thresholds_host, int n_thresholds,
                             int quantile, int init_with_max, uint64_t *segs_dev, void *stream);

/* The host half of bsmi_agglomerate_hist_u8 on a region graph given by the caller (no GPU involved): n_nodes nodes, edges
 * (edge_u[e] < edge_v[e], each pair once) with their 256-bin affinity histograms hist [n_edges][256] (modified); for every
 * threshold (ascending) roots_out + t * n_nodes receives the smallest node of each node's cluster after mergeUntil.     */
int bsmi_agglomerate_hist_graph(uint32_t n_nodes, uint32_t n_edges, const uint32_t *edge_u, const uint32_t *edge_v,
                                uint32_t *hist, int quantile, int init_with_max, const float *thresholds,
                                int n_thresholds, uint32_t *roots_out);

/* Blockwise fragment post-processing (reference post/blockwise/watershed_frags.py:148-156 filter_avg_fragments,
 * :188-192 remove_small_objects, :221-224 crop to the write ROI + skimage.measure.label + global id offset).
 * frags_dev (the read-ROI fragments of bsmi_ws_fragments_u8) is filtered IN PLACE: a fragment is removed
 * if the mean of its 3-channel average affinity (u8/255) is < filter_value (skipped when <= 0) or if it has
 * fewer than min_size voxels (skipped when <= 0).  The crop [crop_offset, +crop_shape) is then relabelled:
 * connected components of equal value under 26-connectivity, numbered id_offset+1.. in raster order of
 * their first voxel; *num_labels_dev receives the count. */
int bsmi_frag_postprocess_u8(bsmi_seg *h, const uint8_t *affs_dev, uint64_t *frags_dev,
                             const int64_t shape[3], double filter_value, int64_t min_size,
                             const int64_t crop_offset[3], const int64_t crop_shape[3],
                             uint64_t id_offset, uint64_t *out_dev, uint64_t *num_labels_dev,
                             void *stream);

/* RAG node attributes of a labelled block (watershed_frags.py:230-246): for labels id_offset+1 ..
 * id_offset+num, size_dev[k] = voxel count and sums_dev[3k..3k+2] = sums of the z, y, x voxel indices
 * (centre of mass = sums / size). */
int bsmi_label_stats(bsmi_seg *h, const uint64_t *labels_dev, const int64_t shape[3], uint64_t id_offset,
                     uint64_t num, uint64_t *size_dev, uint64_t *sums_dev, void *stream);

/* Per-block RAG edge scoring (reference post/blockwise/waterz_agglom.py:106-170): dense relabel of the
 * fragment ids in ascending order (:116-120), waterz.agglomerate(thresholds=[0, threshold],
 * discretize_queue, return_merge_history, return_region_graph) (:131-139), MergeTree replay and per-edge
 * merge score (:153-170; post/merge_tree.py:5-113).  frags_dev may hold arbitrary 64-bit ids (< 2^64-2).
 * Outputs: edges_dev[2e], edges_dev[2e+1] = ids (u < v) of initial RAG edge e, in ascending (u, v) order;
 * scores_dev[e] = score of the merge that first joined u and v, NaN if they never merge below `threshold`;
 * merges_dev[2i], [2i+1] = (surviving id, absorbed id) and merge_scores_dev[i] of merge i (both optional);
 * counts_dev[0..2] = number of edges, merges, nodes.  bsmi_seg_status reports an edge_capacity overflow. */
int bsmi_rag_merge_scores_u8(bsmi_seg *h, const uint8_t *affs_dev, const uint64_t *frags_dev,
                             const int64_t shape[3], float threshold, int discretize_queue,
                             uint64_t *edges_dev, float *scores_dev, uint64_t edge_capacity,
                             uint64_t *merges_dev, float *merge_scores_dev, uint64_t *counts_dev,
                             void *stream);

/* The region graph of a block without the merge loop, for bsmi_rag_merge_scores_host: edges_dev [edge_capacity][2] fragment id
 * pairs (smaller id first) in the order of the device's edge table (NOT sorted, and not the same from run to run:
 * bsmi_rag_merge_scores_host sorts), sums_dev [edge_capacity] affinity sums and pair_counts_dev [edge_capacity] voxel-pair counts
 * of their faces, counts_dev[0..2] = number of edges, 0, nodes.  bsmi_seg_status reports an edge_capacity overflow (counts_dev[0]
 * then says how many entries the block needs).  Four launches; the ordered form behind bsmi_rag_merge_scores_u8 is sixty. */
int bsmi_rag_graph_u8(bsmi_seg *h, const uint8_t *affs_dev, const uint64_t *frags_dev, const int64_t shape[3],
                      uint64_t *edges_dev, uint64_t *sums_dev, uint32_t *pair_counts_dev, uint64_t edge_capacity,
                      uint64_t *counts_dev, void *stream);
/* waterz_agglom.py:106-170 on the host for n_graphs graphs of bsmi_rag_graph_u8 (host copies) side by side on up to n_threads
 * threads (<= 0: 24), largest first.  Every graph is first brought into ascending (id, id) order IN PLACE (edges, sums and
 * pair_counts permuted together), then agglomerated to `threshold` with OneMinus<MeanAffinity> and a `discretize_queue`-bin queue;
 * every edge's score = the score at which its two regions merged (NaN: never) -> scores[g][e], e in the sorted order.  Same
 * results as bsmi_rag_merge_scores_u8. */
int bsmi_rag_merge_scores_host(int n_graphs, const uint64_t *n_edges, uint64_t *const *edges, uint64_t *const *sums,
                               uint32_t *const *pair_counts, float threshold, int discretize_queue, float *const *scores,
                               int n_threads);
/* The same with the queue's bin rule as an argument.  waterz's `discretize_queue` binning (reference
 * post/blockwise/waterz_agglom.py:136; waterz is an unpinned git dependency that is not in /root/reference) cannot be checked
 * in this repository, so the rule is a documented choice (segment config key `queue_bins_formula`):
 * BSMI_QUEUE_BINS_N_MINUS_1 (default, what the oracle and the device loop do) bin = (int)(score * (N - 1));
 * BSMI_QUEUE_BINS_N bin = min(N - 1, (int)(score * N)).  tools/gen_goldens_waterz.py produces the vectors that decide. */
#define BSMI_QUEUE_BINS_N_MINUS_1 0
#define BSMI_QUEUE_BINS_N 1
int bsmi_rag_merge_scores_host_rule(int n_graphs, const uint64_t *n_edges, uint64_t *const *edges, uint64_t *const *sums,
                                    uint32_t *const *pair_counts, float threshold, int discretize_queue, int bin_rule,
                                    float *const *scores, int n_threads);

/* Epsilon agglomeration of a block's fragments IN PLACE (reference post/blockwise/watershed_frags.py:158-177:
 * waterz.agglomerate(thresholds=[epsilon], fragments, "OneMinus<MeanAffinity>", discretize_queue=256), result written
 * back into the fragments): every fragment takes the id of its cluster, the smallest id among the fragments merged
 * into it.  Same region graph and merge loop as bsmi_rag_merge_scores_u8. */
int bsmi_rag_agglomerate_u8(bsmi_seg *h, const uint8_t *affs_dev, uint64_t *frags_dev, const int64_t shape[3],
                            float threshold, int discretize_queue, void *stream);

/* Affinity sum (uint8 units) and voxel-pair count of every initial RAG edge of the last bsmi_rag_merge_scores_u8 call
 * on this handle, in the order of its edges_dev: what waterz's region graph {u, v, score} is computed from
 * (score = 1 - sum / (255 count)); also lets a caller contract the graph along the merge history. */
int bsmi_rag_edge_stats(bsmi_seg *h, uint64_t *sums_dev, uint64_t *counts_dev, uint64_t capacity, void *stream);

/* LUT relabel (volara Relabel + LUT, post/watershed.py:187-202): out[p] = vals[k] where keys[k] == in[p]
 * (keys ascending); 0 stays 0; ids without a key are copied.  in_dev == out_dev is allowed. */
int bsmi_lut_relabel(int device, const uint64_t *in_dev, uint64_t n, const uint64_t *keys_dev,
                     const uint64_t *vals_dev, uint64_t m, uint64_t *out_dev, void *stream);
/* The same with n_columns value columns at once (one segmentation per threshold): vals_dev [n_columns][m], out_dev
 * [n_columns][n]; one look-up per run of equal ids serves every column.  out_dev must not overlap in_dev. */
int bsmi_lut_relabel_multi(int device, const uint64_t *in_dev, uint64_t n, const uint64_t *keys_dev,
                           const uint64_t *vals_dev, uint64_t m, int n_columns, uint64_t *out_dev, void *stream);

/* Global thresholded connected components of the scored RAG on the HOST (plain host pointers; reference
 * post/watershed.py:182 calls funlib.segment.graphs.impl.connected_components, a host C++ routine).
 * nodes strictly ascending; an edge joins its endpoints when score <= threshold; components[i] = smallest
 * node id of node i's component.  Edges naming unknown nodes are ignored. */
int bsmi_connected_components(const uint64_t *nodes, uint64_t n, const uint64_t *edges,
                              const float *scores, uint64_t m, float threshold, uint64_t *components);
/* The same for several thresholds in one pass (reference post/watershed.py:177-186 loops over the thresholds): the node
 * look-up of the edges is done once, on a few host threads, and the unions of a lower threshold carry over to the higher
 * ones.  components: [n_thresholds][n], row k for thresholds[k]. */
int bsmi_connected_components_multi(const uint64_t *nodes, uint64_t n, const uint64_t *edges,
                                    const float *scores, uint64_t m, const float *thresholds,
                                    int n_thresholds, uint64_t *components);

/* Thresholded-affinity connected components (`bs segment --cc`; reference post/cc.py:7-74 called from
 * post/connected_components.py:77-80, debris removal :97-101).  Voxel p is linked with its +z / +y / +x neighbour when
 * affs[d][p] > cut (cut = the uint8 value equivalent to the reference's float threshold: the largest v with
 * !(v / 255.0f > threshold)).  frags_dev: labels 1.. in raster order of each component's first voxel; seg_dev
 * (optional): the same with components of fewer than min_size voxels removed; *num_labels_dev = component count. */
int bsmi_cc_affs_u8(bsmi_seg *h, const uint8_t *affs_dev, const int64_t shape[3], int cut, int64_t min_size,
                    uint64_t *frags_dev, uint64_t *seg_dev, uint64_t *num_labels_dev, void *stream);

/* ---- mutex watershed (`bs segment --mws`) ------------------------------------------------------------------
 * Replaces mwatershed.agglom as the reference calls it (post/mws.py:51-56; the package is third party and absent:
 * restated from Wolf et al., "The Mutex Watershed", parity unpinned).  affs_dev: f64 [n_offsets][D][H][W] on the
 * device, already shifted (w > 0 attractive, w < 0 repulsive, 0 / NaN: no edge); offsets / strides: host
 * int32 [n_offsets][3] (strides NULL = every voxel; random_seed != 0 = the "randomized_strides" form: an edge is kept
 * with probability 1 / prod(stride)).  Edges in order of |w| descending, ties (channel, voxel) ascending.
 * labels_dev: u64 [D][H][W], 1 + smallest voxel index of the cluster.  Synchronises `stream` (the sweep over the
 * sorted edges runs on the host: it is sequential by definition). */
int bsmi_mws_agglom_f64(int device, const double *affs_dev, int n_offsets, const int32_t *offsets,
                        const int32_t *strides, uint32_t random_seed, const int64_t shape[3],
                        uint64_t *labels_dev, void *stream);

/* Mutex watershed on a graph, HOST pointers (volara GraphMWS -> mwatershed.cluster, reference
 * post/watershed_mutex.py:155-161): edges u64 [m][2] of node indices < n_nodes, scores f64 [m] (sign as above),
 * labels_out[i] = 1 + smallest node index of node i's cluster. */
int bsmi_mws_cluster(uint64_t n_nodes, const uint64_t *edges, const double *scores, uint64_t m,
                     uint64_t *labels_out);

/* Affinity statistics between adjacent fragments over a neighbourhood (volara AffAgglom, reference
 * post/watershed_mutex.py:143-153, scores={"zyx_aff": neighborhood}).  affs_dev: u8 [n_offsets][D][H][W]; dense_dev:
 * u64 [D][H][W] of dense fragment indices 1..n < 2^32 (0 = background); for every unordered pair of different
 * fragments joined by some (p, p + offset_k): pairs_out[i] = {smaller, larger} (HOST, ascending), sums_out[i] = sum
 * of the affinity bytes, counts_out[i] = number of such voxel pairs.  *n_pairs is always set; BSMI_ERR_INVALID if
 * it exceeds `capacity`. */
int bsmi_frag_pair_affinity_u8(int device, const uint8_t *affs_dev, int n_offsets, const int32_t *offsets,
                               const uint64_t *dense_dev, const int64_t shape[3], uint64_t capacity,
                               uint64_t *pairs_out, uint64_t *sums_out, uint64_t *counts_out,
                               uint64_t *n_pairs, void *stream);

/* Label table of a block (`bs refine` statistics: reference refine.py:98-109 `_global_sizes`, :228-250 z extents):
 * the distinct non-zero ids of labels_dev in ascending order with their voxel counts and first / last z slice
 * (z0 = global index of the block's first slice).  *n_dev = number of ids (<= capacity, else bsmi_seg_status
 * reports an overflow).  The filters themselves mask / remap through bsmi_lut_relabel. */
int bsmi_label_table_u64(bsmi_seg *h, const uint64_t *labels_dev, const int64_t shape[3], int64_t z0,
                         uint64_t *ids_dev, uint64_t *counts_dev, int32_t *zmin_dev, int32_t *zmax_dev,
                         uint64_t capacity, uint64_t *n_dev, void *stream);

/* fragments_in_xy = 0 (reference post/ws.py:98-110) floods the block from ONE priority queue.  on = 1: that flood runs on the
 * host (csrc/flood_host.cpp: 0.16 s per 128^3 block instead of 12.8 s for the device's single-wave replay) and
 * bsmi_ws_fragments_seeds_u8 returns when the fragments are written (the Python engines switch it on); 0 (the handle's
 * default): the device loop, asynchronous like every other call. */
int bsmi_seg_set_host_flood(bsmi_seg *h, int on);

/* status of the asynchronous seg calls on this handle since the previous bsmi_seg_status (an overflow of any of
 * them is remembered on the device until it is read here; synchronises `stream`): BSMI_OK or BSMI_ERR_OVERFLOW.
 * After an overflow the outputs of that call are undefined. */
int bsmi_seg_status(bsmi_seg *h, void *stream);

/* Batches: the blocks of a blockwise stage served by ONE launch per kernel instead of a chain of launches per block on a stream
 * each (whose concurrency is the number of hardware queues the runtime grants: 4 by default).  A batch object is made from n
 * (1..32) workspaces of one device; block i of a call uses workspace i (its F and C buffers in a fragments call, its G buffers in
 * a graph call: see the handle's rule in csrc/seg_internal.h), so calls on one batch object belong to one stream, and no
 * single-handle call may run on one of its workspaces meanwhile.  Overflows stay per workspace: bsmi_seg_status(handle i).
 * The calls are asynchronous, never synchronise with the host and read no host memory after they return.
 * Served: fragments_in_xy = 1 on slices of the LDS path (H^2 + W^2 < 65535 and the seed kernel's arrays within 158 KiB, e.g. up to
 * 160 x 160), all n_blocks blocks of ONE shape.  Everything else returns BSMI_ERR_INVALID and is the single-handle calls' to do. */
typedef struct bsmi_seg_batch bsmi_seg_batch;
typedef struct {
  const uint8_t *affs_dev;   /* [3][shape] */
  uint64_t *frags_dev;       /* [shape]: the fragments before the crop (filtered in place), as bsmi_ws_fragments_u8 writes them */
  uint64_t *max_id_dev;      /* [1] */
  uint64_t *labels_dev;      /* [crop_shape]: bsmi_frag_postprocess_u8's out_dev */
  uint64_t *num_labels_dev;  /* [1] */
  uint64_t id_offset;
  uint64_t *size_dev;        /* [stats_num], bsmi_label_stats of labels_dev */
  uint64_t *sums_dev;        /* [stats_num][3] */
} bsmi_batch_frag_args;
typedef struct {
  const uint8_t *affs_dev;
  const uint64_t *frags_dev;
  uint64_t *edges_dev;
  uint64_t *sums_dev;
  uint32_t *pair_counts_dev;
  uint64_t *counts_dev;
  uint64_t edge_capacity;
} bsmi_batch_graph_args;
int bsmi_seg_batch_create(bsmi_seg *const *handles, int n, bsmi_seg_batch **out);
int bsmi_seg_batch_destroy(bsmi_seg_batch *b);  /* before the handles it was made from */
/* per block: bsmi_ws_fragments_u8, bsmi_frag_postprocess_u8 (filter_value, min_size, crop, id_offset) and bsmi_label_stats
 * (id_offset, stats_num) on the crop, bit for bit */
int bsmi_seg_batch_fragments_u8(bsmi_seg_batch *b, int n_blocks, const bsmi_batch_frag_args *args, const int64_t shape[3],
                                int fragments_in_xy, int min_seed_distance, double filter_value, int64_t min_size,
                                const int64_t crop_offset[3], const int64_t crop_shape[3], uint64_t stats_num, void *stream);
/* per block: bsmi_rag_graph_u8 */
int bsmi_seg_batch_rag_graph_u8(bsmi_seg_batch *b, int n_blocks, const bsmi_batch_graph_args *args, const int64_t shape[3],
                                void *stream);

/* ---- evaluation ---- */
/* `bs evaluate` (evaluate.py:39-101): affinity error maps of a segmentation against the network's own affinities
 * (eval/compute_errors.py:25-223, gp/add_aff_errors.py) and the (gt, seg) contingency table behind Rand / VOI
 * (eval/compute_metrics.py:73-122, funlib.evaluate.rand_voi).  The handle holds the pair table (three open-addressing tables
 * of pair_capacity slots: gt ids, seg ids, (gt slot, seg slot) pairs with u64 counts), an overflow flag, and the f32 scratch of
 * the error pass (grown on demand; growing synchronises the stream).  pair_capacity: a power of two in [2, 2^31]. */
typedef struct bsmi_eval bsmi_eval;
int bsmi_eval_create(int device, uint64_t pair_capacity, bsmi_eval **out);
int bsmi_eval_destroy(bsmi_eval *h);

/* Affinity errors of a tile of Scan chunks (a layer of chunks across the ROI, or more), AddAffErrors._create_diff /
 * _create_mask with the per-chunk normalisation, in the reference's f32 arithmetic (no contraction):
 *   s_e  = seg[v] == seg[v + offset_e] && seg[v] != 0;  p_e = float(pred[e][v]) * float(1/255)
 *   diff = ((s_0 - p_0)^2 + (s_1 - p_1)^2) + ...  (* float(mask[v]) when mask_dev is given)
 *   d    = diff / max(diff over the chunk) (0 when that is 0);  error_map = u8(trunc(d * 255));  error_mask = floor < d < ceil
 * tile_shape (tz, ty, tx): the tile; pred_dev u8 [n_channels][tz][ty][tx], mask_dev u8 [tz][ty][tx] or NULL, the two outputs
 * u8 [tz][ty][tx].  seg_dev u64 [seg_shape]: the segmentation around the tile, seg_origin = position of its first voxel relative
 * to the tile's first voxel (<= 0); it must hold every v + offset_e (zeros where the dataset ends), else BSMI_ERR_INVALID.
 * offsets: host int32 [n_channels][3] (n_channels <= 16), either sign.  chunk_shape: the chunk's extent per axis (clamped
 * to the tile): along each axis chunks start at 0, c, 2c, ... and the last one is moved back to end at the tile's end; a voxel
 * takes the value of the last chunk covering it.  At most 65535 chunks per tile.  hist_dev u64 [257] accumulates (not cleared): [i] +=
 * voxels with error_map == i, [256] += voxels with error_mask == 1, over the slices z < count_z_end only (the caller's next
 * layer rewrites the rest).  25 bytes of HBM per voxel at 6 channels with a mask (f32 diff stored between two kernels). */
int bsmi_eval_aff_errors_u8(bsmi_eval *h, const uint64_t *seg_dev, const int64_t seg_shape[3], const int64_t seg_origin[3],
                            const uint8_t *pred_dev, int n_channels, const int64_t tile_shape[3], const uint8_t *mask_dev,
                            const int32_t *offsets, const int64_t chunk_shape[3], float floor_, float ceil_, int64_t count_z_end,
                            uint8_t *error_map_dev, uint8_t *error_mask_dev, uint64_t *hist_dev, void *stream);

/* LSD errors of a tile of Scan chunks (gp/add_lsd_errors.py as eval/compute_errors.py:149-177 calls it), chunk by chunk as
 * the reference's `process` does, over the chunk grown by `margin` voxels per side (region G; the reference requests
 * chunk + (4, 100, 100), margin (2, 50, 50); (0, 0, 0) is the bare chunk):
 *   a    = the 10 local shape descriptors of the segmentation over G (gaussian mode, all components), from the label array
 *          L = G grown by `context` = floor(3 sigma / voxel_size) voxels per side: windows on the sub-grid L[::downsample]
 *          anchored at L's first voxel, weights as scipy.ndimage.gaussian_filter(mode="constant", truncate=3.0) builds them,
 *          float64 accumulation, variances clamped at 1e-3, clipped to [0, 1], 0 on background (the arithmetic of
 *          bsmi_train_lsd_targets; the lsd package is restated, parity unpinned)
 *   diff = ((a_0 - p_0)^2 + (a_1 - p_1)^2) + ... over the 10 channels in f32 without contraction, p_c = float(pred[c]) *
 *          float(1/255), (* float(mask) when mask_dev is given);  d = diff / max(diff over G) (0 when that is 0)
 *   raw  = floor < d < ceil over G; opened in the plane by the L1 diamond of radius 4 (= binary_erosion then binary_dilation
 *          with the 4-neighbour cross, iterations = 4), then closed along z by the 3-column, every step with 0 outside G
 *   error_map = u8(trunc(d * 255)), error_mask = the closed mask, both cropped to the chunk
 * seg_dev: u64 [seg_shape], seg_origin = its first voxel relative to the tile's (<= -(margin + context)); it must hold the
 * tile grown by margin + context (zeros beyond the dataset).  pred_dev u8 [10][tile + 2 margin], mask_dev u8 [tile + 2 margin]
 * or NULL (zeros beyond their datasets).  chunk + 2 margin and context must be multiples of downsample on every axis, and the
 * window radii round(3 sigma / (voxel_size downsample)) must fit the descriptor kernel's LDS window ((2 + 2 rz) (8 + 2 ry)
 * (16 + 2 rx) cells of 4 bytes plus the weight tables in 71 KiB), else BSMI_ERR_INVALID.  downsample is 1 or 2.  Chunk placement, ownership of
 * overlapped voxels, hist_dev and count_z_end as in bsmi_eval_aff_errors_u8.  Labels become 32-bit ids through an id table of
 * the handle's pair_capacity slots; more distinct labels than it holds set the overflow flag (bsmi_eval_status).  The chunks
 * are processed in groups whose scratch (per chunk 4 B per sub-grid cell of L and 7 B per voxel of G) stays below
 * scratch_limit_bytes; a single chunk above it is BSMI_ERR_INVALID.
 * Debug outputs (NULL in production), per chunk over its region G, chunks in the order (jz * ncy + jy) * ncx + jx:
 * debug_desc_dev f32 [chunks][10][G], debug_diff_dev f32 [chunks][G] (before normalisation), debug_max_dev f32 [chunks],
 * debug_raw_mask_dev u8 [chunks][G] (before the morphology). */
int bsmi_eval_lsd_errors_u8(bsmi_eval *h, const uint64_t *seg_dev, const int64_t seg_shape[3], const int64_t seg_origin[3],
                            const uint8_t *pred_dev, const uint8_t *mask_dev, const int64_t tile_shape[3],
                            const int64_t chunk_shape[3], const int64_t margin[3], const int64_t context[3], const float sigma[3],
                            const float voxel_size[3], int downsample, float floor_, float ceil_, int64_t count_z_end,
                            uint64_t scratch_limit_bytes, uint8_t *error_map_dev, uint8_t *error_mask_dev, uint64_t *hist_dev,
                            float *debug_desc_dev, float *debug_diff_dev, float *debug_max_dev, uint8_t *debug_raw_mask_dev,
                            void *stream);

/* Adds a tile's (gt, seg) voxel pairs to the handle's pair table (reset != 0 empties it first).  gt_dev, seg_dev u64
 * [shape]; mask_dev u8 [shape] or NULL: both ids are multiplied by the mask value first, wrapping at 2^64, as the reference
 * does.  Voxels whose (masked) gt id is 0 are left out; seg id 0 is an ordinary label.  Runs of equal pairs along x are
 * counted within a wave before the atomics; counts are exact, so the table does not depend on the order of the atomics.
 * A full table sets the overflow flag (bsmi_eval_status); the counts are then incomplete. */
int bsmi_eval_pairs_u64(bsmi_eval *h, const uint64_t *gt_dev, const uint64_t *seg_dev, const uint8_t *mask_dev,
                        const int64_t shape[3], int reset, void *stream);

/* Reads the pair table out: (gt_out_dev[i], seg_out_dev[i], count_out_dev[i]) for i < *n_dev (u64 on the device), in no
 * particular order.  More than out_capacity pairs set the overflow flag. */
int bsmi_eval_pairs_read(bsmi_eval *h, uint64_t *gt_out_dev, uint64_t *seg_out_dev, uint64_t *count_out_dev,
                         uint64_t out_capacity, uint64_t *n_dev, void *stream);

/* BSMI_OK, or BSMI_ERR_OVERFLOW if a table of this handle overflowed since the previous call (the flag is cleared here).
 * Synchronises `stream`. */
int bsmi_eval_status(bsmi_eval *h, void *stream);

/* ---- label-preserving morphology (`bs refine morph`) ----------------------------------------------------------
 * Replaces fastmorph as the reference calls it (refine.py:310-344 `_apply_morph`; the package is third party and absent:
 * the rule below is this project's own, restated in tests/morph_ref.py, parity unpinned).
 * The array A that one operation sees is the whole volume [D][H][W] with a 3 x 3 x 3 stencil, or, with xy != 0, every z
 * section on its own with a 3 x 3 stencil (all sections in one launch).
 *   dilate (fastmorph.dilate, background_only=True, refine.py:330-332): a non-zero voxel keeps its id; a zero voxel takes
 *     the most frequent non-zero id among the stencil voxels inside A, ties to the smallest id, 0 if there is none.
 *   erode (fastmorph.erode, erode_border=True, refine.py:333-335): a non-zero voxel keeps its id only if every stencil
 *     voxel holds the same id; positions outside A count as background, so ids on A's faces always go.
 * `iterations` (1..255) applies the step that many times, each on the previous result; opening and closing
 * (refine.py:336-341) are two calls.  tmp_dev: ping-pong buffer of the volume's size, may be NULL for one iteration.
 * in_dev is never written; in_dev, out_dev and tmp_dev must differ (BSMI_ERR_INVALID).  One launch per iteration,
 * 16 bytes of HBM per voxel each; asynchronous on `stream`. */
#define BSMI_MORPH_DILATE 0
#define BSMI_MORPH_ERODE 1
int bsmi_label_morph_u64(int device, const uint64_t *in_dev, const int64_t shape[3], int op, int iterations, int xy,
                         uint64_t *out_dev, uint64_t *tmp_dev, void *stream);

/* fill_holes (stands in for fastmorph.fill_holes_v2(fix_borders=two_d, merge_threshold=0.95), refine.py:317-326).
 * Components are maximal face-connected sets of voxels of A with equal id (6-neighbourhood, 4-neighbourhood with xy != 0),
 * id 0 included.  A component with a voxel on a face of A (an edge of its section with xy) is left alone.  For every
 * other component C the faces between a voxel of C and a face-neighbour outside C are counted per neighbouring id; T is
 * their total, L the non-zero neighbouring id with the largest count n_L (ties to the smallest id); if
 * BSMI_MORPH_MERGE_DEN * n_L >= BSMI_MORPH_MERGE_NUM * T (0.95 in integers) every voxel of C takes the id L.  All
 * decisions are taken on the input and applied at once (no chaining).
 * scratch_dev: bsmi_label_fill_holes_scratch_bytes(shape, table_capacity) bytes on the device; table_capacity: slots
 * (a power of two in [2, 2^31]) of the (component, neighbouring id) face table and of its id table.  Fewer than 2^32 - 1
 * voxels per call.  The decision runs on the host from the read-out table, so the call synchronises `stream` and a full
 * table comes back from the call itself as BSMI_ERR_OVERFLOW (out_dev is then undefined; call again with a larger
 * table).  *n_filled (optional, host): the number of components that changed id. */
#define BSMI_MORPH_MERGE_NUM 19ull
#define BSMI_MORPH_MERGE_DEN 20ull
size_t bsmi_label_fill_holes_scratch_bytes(const int64_t shape[3], uint64_t table_capacity);
int bsmi_label_fill_holes_u64(int device, const uint64_t *in_dev, const int64_t shape[3], int xy, uint64_t *out_dev,
                              void *scratch_dev, size_t scratch_bytes, uint64_t table_capacity, uint64_t *n_filled,
                              void *stream);

/* ---- volume utilities (`bs utils`: mask, scale_pyramid, bbox) -------------------------------
 * Raw mask (reference data/mask.py:15-30): the binary closing of every z section of in_dev u8 [D][H][W] on its own, on
 * in != 0, by the disk dx^2 + dy^2 <= radius^2 (1 <= radius <= 16), written as 0 / 1 to out_dev.  The closing is that of
 * the section zero-extended to the infinite plane, restricted to the section:
 *   out(p) = AND_{q in p + disk} OR_{s in q + disk} x0(s)
 * i.e. the dilation is evaluated on the section grown by `radius` on every side before it is eroded (equal to skimage's
 * binary_closing of the section padded with 2 * radius zeros; restated in tests/utils_ref.py).
 * work_dev: bsmi_mask_closing_work_bytes(shape, radius) bytes on the device, 8-byte aligned (the packed dilation; 0 from
 * that call = bad arguments).  in_dev is never written; in_dev, out_dev and work_dev must differ (BSMI_ERR_INVALID).  Two
 * launches, asynchronous on `stream`. */
size_t bsmi_mask_closing_work_bytes(const int64_t shape[3], int radius);
int bsmi_mask_closing_disk_u8(int device, const uint8_t *in_dev, const int64_t shape[3], int radius, uint8_t *out_dev,
                              void *work_dev, size_t work_bytes, void *stream);

/* One level of a scale pyramid (reference data/scale_pyramid.py:31-56) over [D][H][W] arrays.  Output voxel o covers the
 * input window [o * k - lead, o * k - lead + k) per axis (k = factor, 0 <= lead < k: how far the output grid's origin lies
 * before the input's, in input voxels); input positions outside in_shape count as 0.
 *   bsmi_downscale_mean (itemsize 1 | 2: u8, u16; prod k <= 65536 so that the u32 sum is exact):
 *     out[o] = (sum of the window) / prod k, rounded down -- block_reduce(np.mean) with zero fill, stored as an integer.
 *   bsmi_rescale_sample (itemsize 1, 2, 4, 8):
 *     BSMI_RESCALE_DOWN: out[o] = in[o * k + k / 2 - lead] (0 outside): in_data[slice(k // 2, None, k)].
 *     BSMI_RESCALE_UP:   out[o] = in[o / k]: np.repeat.  lead must be 0 and out_shape <= in_shape * k.
 * in_dev is never written and must differ from out_dev.  Asynchronous on `stream`. */
#define BSMI_RESCALE_DOWN 0
#define BSMI_RESCALE_UP 1
int bsmi_downscale_mean(int device, const void *in_dev, int itemsize, const int64_t in_shape[3], const int32_t factor[3],
                        const int32_t lead[3], void *out_dev, const int64_t out_shape[3], void *stream);
int bsmi_rescale_sample(int device, const void *in_dev, int itemsize, const int64_t in_shape[3], const int32_t factor[3],
                        const int32_t lead[3], int mode, void *out_dev, const int64_t out_shape[3], void *stream);

/* Bounding box of the non-zero voxels (reference data/bbox.py:45, find_objects(arr > 0); elements are read as unsigned
 * integers of `itemsize` 1, 2, 4 or 8 bytes).  box_dev int64 [6] = (min z, y, x, max z, y, x): the call merges the
 * extremes of (z, y, x) + origin over this array's non-zero voxels into what box_dev already holds, so a volume can be
 * streamed tile by tile; the caller initialises it to (INT64_MAX x 3, -1 x 3), which an all-zero volume leaves as it is.
 * Asynchronous on `stream`. */
int bsmi_nonzero_bbox(int device, const void *in_dev, int itemsize, const int64_t shape[3], const int64_t origin[3],
                      int64_t *box_dev, void *stream);

/* ---- synthetic labels of the second-stage setups (csrc/synth.hip; reference gp/create_labels.py,
 * gp/custom_grow_boundary.py, gp/obfuscate_labels.py; the rules in full: DESIGN.md section 7i, tests/synth_ref.py) ----
 * Every random scalar is drawn by the caller.  Volumes are [D][H][W]; a raster index is (z * H + y) * W + x.  The handle
 * holds the work buffers for volumes of up to max_shape voxels (fewer than 2^31); one handle belongs to one host thread
 * and one stream.  Calls that take a host table or hand back a count wait for the stream; the others are asynchronous.
 *
 * dilate_points: the generated sections of the tubes branch.  points: host int32 [n][3] (z, y, x) set to 1; per section z
 *   a structuring bitmap (host uint32 [D][32], bit c of word r = structure[r][c]) of bitmap_sizes[z] = (rows, columns),
 *   applied iterations[z] (0..10) times as scipy's binary_dilation does: origin at (rows / 2, columns / 2), zero outside
 *   the section.  out_dev: int32 0 / 1.  A section whose two bit planes (2 * H * ceil(W / 32) words) exceed 64 KiB of
 *   LDS is refused with BSMI_ERR_INVALID.
 * label_i32: 26-connected components of equal non-zero values; ids are the raster ranks of the components' first voxels,
 *   from 1 (skimage.measure.label's default on any input).  num_host (may be NULL): the number of components.
 * expand_i32: exact Euclidean feature transform.  A voxel whose squared distance to the nearest non-zero voxel is at
 *   most depth^2 takes that voxel's label -- among equidistant ones the one with the lowest raster index -- the others `fill`.
 * tubes_i32: label -> expand(depth = D, fill = components + 1) -> label, as create_labels.py:134-158.
 * gaussian_f32: three passes (z, y, x) of 2 * radius + 1 taps in float32 with the host weights, border `reflect`
 *   (d c b a | a b c d | d c b a), repeated when the radius exceeds the axis.
 * argmax_filter_f32: pos_dev[p] = raster index of the largest value in the window [-(w / 2), w - 1 - w / 2]^3 around p with
 *   `reflect` border; among equal values the lowest raster index.  Values must not be NaN; -0 counts as +0.
 * basins_f32: voxels ordered by (value, lower raster index wins).  A voxel's parent is its best 6-neighbour if that beats the
 *   voxel, else pos_dev[p] if that is a voxel that beats it, else the voxel is a root; label = raster rank of its chain's
 *   root, from 1.  mask_dev (uint8, may be NULL): voxels outside take 0 and are nobody's neighbour, window position or root.
 * finish_i32: zero the ids divisible by 3 (drop3) and by 5 (drop5), keep every anisotropy-th section (section 0 alone when
 *   anisotropy > D); out_dev int64 [ceil(D / anisotropy) or 1][H][W].
 * grow_boundary_i64: CustomGrowBoundary(only_xy=True, no mask).  steps(z, label) = mix(mix(mix(seed) ^ z) ^ label) %
 *   (max_steps + 1), mix = the 64-bit finaliser of MurmurHash3 (k ^= k >> 33; k *= 0xff51afd7ed558ccd; k ^= k >> 33;
 *   k *= 0xc4ceb9fe1a85ec53; k ^= k >> 33).  A non-zero voxel keeps its label if every voxel of its section within L1
 *   distance steps holds that label (positions outside the section count as equal), else it becomes 0.
 * merge_i64: in the 1 or 2 sections given, label b becomes label a.  stamp_i64: the set bits of a bitmap placed with its
 *   corner at (z, y, x) take `value`.  present_i64: the distinct non-zero ids, unordered, into ids_dev (int64
 *   [capacity]) and their number into *count_host; BSMI_ERR_OVERFLOW beyond capacity or 32768 ids.
 * split_i64: mask = labels == id; field = squared Euclidean distance to the nearest voxel outside the mask (the volume's
 *   border is no background; 2^30 where there is none), 0 outside the mask; argmax_filter(window) and basins on the
 *   mask; in the sections given, a mask voxel of fragment k takes k * scale.  num_host (may be NULL): the fragments. */
typedef struct bsmi_synth bsmi_synth;
int bsmi_synth_create(int device, const int64_t max_shape[3], bsmi_synth **out);
int bsmi_synth_destroy(bsmi_synth *h);
int bsmi_synth_dilate_points(bsmi_synth *h, const int64_t shape[3], const int32_t *points, int n_points, const uint32_t *bitmaps,
                             const int32_t *bitmap_sizes, const int32_t *iterations, int32_t *out_dev, void *stream);
int bsmi_synth_label_i32(bsmi_synth *h, const int32_t *in_dev, const int64_t shape[3], int32_t *out_dev, uint64_t *num_host, void *stream);
int bsmi_synth_expand_i32(bsmi_synth *h, const int32_t *labels_dev, const int64_t shape[3], int depth, int32_t fill, int32_t *out_dev,
                          void *stream);
int bsmi_synth_tubes_i32(bsmi_synth *h, const int32_t *fg_dev, const int64_t shape[3], int32_t *out_dev, uint64_t *num_host, void *stream);
int bsmi_synth_gaussian_f32(bsmi_synth *h, const float *in_dev, const int64_t shape[3], const float *weights, int radius, float *out_dev,
                            void *stream);
int bsmi_synth_argmax_filter_f32(bsmi_synth *h, const float *field_dev, const int64_t shape[3], int window, int32_t *pos_dev, void *stream);
int bsmi_synth_basins_f32(bsmi_synth *h, const float *field_dev, const int32_t *pos_dev, const uint8_t *mask_dev, const int64_t shape[3],
                          int32_t *out_dev, uint64_t *num_host, void *stream);
int bsmi_synth_finish_i32(bsmi_synth *h, const int32_t *in_dev, const int64_t shape[3], int drop3, int drop5, int anisotropy, int64_t *out_dev,
                          void *stream);
int bsmi_synth_grow_boundary_i64(int device, const int64_t *in_dev, const int64_t shape[3], uint64_t seed, int max_steps, int64_t *out_dev,
                                 void *stream);
int bsmi_synth_merge_i64(int device, int64_t *labels_dev, const int64_t shape[3], const int32_t *sections, int n_sections, int64_t a, int64_t b,
                         void *stream);
int bsmi_synth_stamp_i64(int device, int64_t *labels_dev, const int64_t shape[3], int z, int y, int x, const uint32_t *bitmap, int bitmap_h,
                         int bitmap_w, int64_t value, void *stream);
int bsmi_synth_present_i64(bsmi_synth *h, const int64_t *labels_dev, uint64_t n_voxels, int64_t *ids_dev, uint32_t capacity, uint32_t *count_host,
                           void *stream);
int bsmi_synth_split_i64(bsmi_synth *h, int64_t *labels_dev, const int64_t shape[3], int64_t id, int window, const int32_t *sections,
                         int n_sections, int64_t scale, uint64_t *num_host, void *stream);

/* ---- training augmentation: the geometric chain of the first-stage 3-D setups (csrc/augment.hip; reference
 * models/3d_affs/train.py:95-104: SimpleAugment -> DeformAugment -> ShiftAugment; the rules in full: DESIGN.md section
 * 7j, tests/aug_ref.py) ----
 * The three nodes compose into one coordinate map, so a sample costs one coordinate launch and one resampling launch per
 * array.  These are specified rules: parity with gunpowder is in distribution, not draw by draw.  Every random scalar
 * is drawn by the caller.  Stateless, asynchronous on `stream`; volumes are [D][H][W].
 *
 * aug_coords writes s(p), the source coordinate in voxels of the crop, for every voxel p = (z, y, x) of a block of
 * `shape`, as three float32 planes coords_dev [3][D][H][W] (z, y, x), all arithmetic in float32:
 *   r = p + (0, shifts[0][p_z], shifts[1][p_z])            shifts_dev: int32 [2][D] (y, x per section) or NULL (none)
 *   d = r - centre                                         centre = (shape - 1) / 2
 *   t = (l0 * d_z, l1 * d_y + l2 * d_x, l3 * d_y + l4 * d_x) + E(r)
 *                                                          linear = (l0 .. l4) = u * (1, cos, -sin, sin, cos) of a
 *                                                          scaling by u and a rotation about z
 *   E(r): trilinear interpolation of lattice_dev, float32 [3][nz][ny][nx] (component z, y, x in voxels), or 0 when
 *         lattice_dev is NULL.  Per axis g = r * inv_spacing + org, clamped to [0, n - 1]; org = 1 (node 0 lies one spacing
 *         before the block) or 0 on an axis of one node; cell = min(floor(g), max(n - 2, 0)), weight g - cell,
 *         a + w * (b - a) along x, then y, then z.  nz * ny * nx <= 4096 (48 KiB of LDS), else BSMI_ERR_INVALID.
 *   if swap_yx: t_y <-> t_x (needs shape[1] == shape[2], else BSMI_ERR_INVALID)
 *   s = src_centre + (mirror bit a set ? -t_a : t_a)        mirror: bit 0 / 1 / 2 = z / y / x; src_centre: the block's
 *                                                          centre in voxels of the crop
 * aug_sample_* read coords_dev (of coords_shape) at the voxels [region_offset, region_offset + region_shape) -- so one
 * coordinate volume serves the input block, the output block and the LSD region -- and a crop of crop_shape; out_dev has
 * region_shape.  Every index is clamped to the crop: a wrong coordinate can give a wrong sample, never a read outside.
 *   f32_u8:      trilinear, cell floor(s), both corners clamped, a + w * (b - a) along x, y, z; out = (v * 2 - 255) / 255
 *                (v * 2 / 255 - 1 in one rounded division: within half an ulp where s is a voxel centre).
 *   nearest_i64, nearest_u8: crop[clamp(floor(s + 0.5))] per axis, the sum and the floor in float32.
 * A block, a crop or a region holds fewer than 2^31 voxels. */
int bsmi_aug_coords(int device, const int64_t shape[3], const float linear[5], const float centre[3], const float src_centre[3], int mirror,
                    int swap_yx, const int32_t *shifts_dev, const float *lattice_dev, const int32_t lattice_shape[3], const float inv_spacing[3],
                    float *coords_dev, void *stream);
int bsmi_aug_sample_f32_u8(int device, const float *coords_dev, const int64_t coords_shape[3], const int64_t region_offset[3],
                           const int64_t region_shape[3], const uint8_t *crop_dev, const int64_t crop_shape[3], float *out_dev, void *stream);
int bsmi_aug_sample_nearest_i64(int device, const float *coords_dev, const int64_t coords_shape[3], const int64_t region_offset[3],
                                const int64_t region_shape[3], const int64_t *crop_dev, const int64_t crop_shape[3], int64_t *out_dev,
                                void *stream);
int bsmi_aug_sample_nearest_u8(int device, const float *coords_dev, const int64_t coords_shape[3], const int64_t region_offset[3],
                               const int64_t region_shape[3], const uint8_t *crop_dev, const int64_t crop_shape[3], uint8_t *out_dev,
                               void *stream);

/* ---- training augmentation: the intensity chain of raw (csrc/augment_intensity.hip; reference models/3d_mtlsd/train.py:
 * 117-132: NoiseAugment -> IntensityAugment -> GammaAugment -> ImpulseNoiseAugment -> SmoothAugment -> DefectAugment; the
 * rules in full: DESIGN.md section 7k, tests/intensity_ref.py) ----
 * Specified rules, like the geometric chain: parity with gunpowder / skimage is in distribution.  Each node is one call on
 * a float32 block x_dev [D][H][W] with values in [0, 1], changed in place; a node the caller's plan skips is simply not
 * called.  Sections are the z planes.  Stateless, asynchronous on `stream`; fewer than 2^31 voxels, at most 65535 sections.
 *
 *   sample_unit_f32_u8   aug_sample_f32_u8 with out = v / 255 (one rounded division): the chain's input.
 *   noise      x = clip(x + sigma * n, 0, 1), n a standard normal per voxel (below).
 *   section_stats  stats_dev [D][3] = (mean, min, max) of every section.  Deterministic: BSMI_AUG_STAT_PARTS workgroups per
 *              section each reduce a fixed chunk in a fixed order into partials_dev (workspace, [D][BSMI_AUG_STAT_PARTS][3]
 *              floats), which a second launch combines in index order; mean = sum / (H * W).  No atomics.
 *   intensity  x = clip(m_z + (x - m_z) * scale_z + shift_z, 0, 1); m_z = stats[z][0]; scale_dev, shift_dev: float32 [D].
 *   gamma      with a = stats[z][1], b = stats[z][2]: where b - a > 1e-3, x = ((x - a) / (b - a))^gamma_z * (b - a) + a, held to
 *              [a, b]; x = a stays a; otherwise the section is unchanged.  gamma_dev: float32 [D], positive.
 *   impulse    a voxel whose word o2 < threshold (threshold <= 2^32; 2^32: every voxel) becomes (o3 >> 8) * 2^-24.
 *   smooth     separable Gaussian with the caller's normalised taps weights[2 * radius + 1] (host memory), radius <=
 *              BSMI_AUG_MAX_RADIUS, border "reflect" (d c b a | a b c d, repeated where the radius exceeds the axis), passes
 *              along z (x_dev -> tmp_dev, a workspace of the block's size), then y and x (one launch, from a tile staged
 *              with its halo in LDS, tmp_dev -> x_dev); each tap sum runs from tap 0 upwards.
 *   defect     mode_dev int32 [D] or NULL: 0 unchanged, 1 / 2 the section becomes 0 / 1, 3 x = m_z + (x - m_z) * contrast_scale;
 *              then, if final_map, x = 2 x - 1 (the chain's output).
 * Per-voxel random numbers: one Philox4x32-10 call per voxel, key (seed low word, seed high word), counter (linear voxel
 * index, 0, 0, 0), output o0 .. o3; u1 = ((o0 >> 8) + 1) * 2^-24, u2 = (o1 >> 8) * 2^-24, n = sqrt(-2 ln u1) * cospi(2 u2). */
#define BSMI_AUG_STAT_PARTS 16
#define BSMI_AUG_MAX_RADIUS 6
int bsmi_aug_sample_unit_f32_u8(int device, const float *coords_dev, const int64_t coords_shape[3], const int64_t region_offset[3],
                                const int64_t region_shape[3], const uint8_t *crop_dev, const int64_t crop_shape[3], float *out_dev,
                                void *stream);
int bsmi_aug_noise_f32(int device, const int64_t shape[3], float *x_dev, uint64_t seed, float sigma, void *stream);
int bsmi_aug_section_stats_f32(int device, const int64_t shape[3], const float *x_dev, float *partials_dev, float *stats_dev, void *stream);
int bsmi_aug_intensity_f32(int device, const int64_t shape[3], float *x_dev, const float *stats_dev, const float *scale_dev,
                           const float *shift_dev, void *stream);
int bsmi_aug_gamma_f32(int device, const int64_t shape[3], float *x_dev, const float *stats_dev, const float *gamma_dev, void *stream);
int bsmi_aug_impulse_f32(int device, const int64_t shape[3], float *x_dev, uint64_t seed, uint64_t threshold, void *stream);
int bsmi_aug_smooth_f32(int device, const int64_t shape[3], float *x_dev, float *tmp_dev, const float *weights, int radius, void *stream);
int bsmi_aug_defect_f32(int device, const int64_t shape[3], float *x_dev, const float *stats_dev, const int32_t *mode_dev,
                        float contrast_scale, int final_map, void *stream);

/* ---- training augmentation of the 2-D setups: the geometric chain, a whole batch per launch (csrc/augment2d.hip; reference
 * models/2d_mtlsd/train.py:112-122 and its 2d_affs / 2d_lsd siblings: SimpleAugment -> DeformAugment(spatial_dims=2) ->
 * ShiftAugment under gp.Stack(10); the rules in full: DESIGN.md section 7l, tests/aug2d_ref.py) ----
 * A step is S independent draws of one output section each, every draw with its own plan and its own crop, so the launches
 * read one table of per-draw descriptors: ONE coordinate launch for all draws and all K adjacent sections of raw, ONE
 * resampling launch per array for all draws.  Specified rules, like the 3-D chain: parity with gunpowder is in
 * distribution.  Every random scalar is drawn by the caller.  Stateless, asynchronous on `stream`.
 *
 * With I = input_shape (H, W), c = (I - 1) / 2, F_lo = frame_offset (<= 0 per axis) and F = frame_shape (the frame
 * [F_lo, F_lo + F) contains the input section [0, I): it is the union of the input section and the labels window, which may
 * be the larger), aug2d_coords writes, for every draw s, section k and frame pixel (y, x) -- y, x in the input section's own
 * pixels, possibly outside [0, I) -- the source coordinate in pixels of the draw's crop, all arithmetic in float32:
 *   r = (y + shifts[s][0][k], x + shifts[s][1][k])         shifts_dev: int32 [S][2][K] or NULL (none)
 *   d = r - c
 *   t = (a0 * d_y + a1 * d_x, a2 * d_y + a3 * d_x) + E(r)   a = u * (cos, -sin, sin, cos)
 *   E(r): bilinear interpolation of the draw's lattice, float32 [2][n_y][n_x] (component y, x in pixels) at lattice_offset
 *         floats inside lattice_dev, or 0 when n = 0 x 0.  Per axis g = (r - F_lo) * inv_spacing + 1 (node j lies at F_lo +
 *         (j - 1) * spacing), clamped to [0, n - 1]; cell = min(floor(g), n - 2), weight g - cell, a + w * (b - a) along x,
 *         then y.  n_y * n_x <= 4096 (32 KiB of LDS per draw), else BSMI_ERR_INVALID.
 *   if swap: t_y <-> t_x (needs H == W, else BSMI_ERR_INVALID)
 *   s = src + (mirror bit set ? -t : t) per axis            src: the input section's centre in pixels of the crop
 * coords_dev: float32 [S][K][2][F_h][F_w].  z is never interpolated: the z mirror only makes section k of raw read section
 * K - 1 - k of the crop.
 * aug2d_sample_* read the planes at the frame pixels [region_offset, region_offset + region_shape) (an offset inside the
 * frame, not the input section) and gather from the draw's crop, every index clamped to that crop:
 *   f32_u8:      crops_dev holds, per draw, K sections [K][crop_h][crop_w] at pixel K * crop_offset.  Bilinear in the plane
 *                of section k_src through the coordinates of section k: cell floor(s), both corners clamped, a + w * (b - a)
 *                along x, then y; out = (v * 2 - 255) / 255 into out_dev float32 [K][S][r_h][r_w], what the trainer reads.
 *   nearest_i64, nearest_u8: one section per draw at pixel crop_offset; crop[clamp(floor(s + 0.5))] per axis, the sum and the
 *                floor in float32, through the coordinates of section K / 2; out_dev [S][r_h][r_w].
 * The table is passed twice: `draws` in host memory, which every call checks (S < 1, K < 1, more than 65535 (draw, section)
 * pairs, a lattice of more than 4096 nodes or beyond lattice_floats, a swap of a non-square section, a crop beyond
 * crop_pixels -- the pixels of crops_dev --, 2^31 coordinates / outputs or more: BSMI_ERR_INVALID), and `draws_dev`, the
 * same bytes in device memory, which the kernels read.  Uploading the table is the caller's: once per batch for the four
 * calls. */
typedef struct bsmi_aug2d_draw {
  float a[4];           /* A = u R(theta), row-major 2 x 2 */
  float src[2];         /* c_src (y, x) */
  float inv_spacing[2]; /* 1 / (node spacing in pixels), (y, x) */
  int32_t flags;        /* bit 0 / 1 / 2: mirror z / y / x; bit 3: swap y <-> x, applied before the mirrors */
  int32_t n[2];         /* lattice nodes (n_y, n_x); 0 x 0: no elastic term */
  int32_t lattice_offset; /* of this draw's [2][n_y][n_x] floats in the packed lattice buffer */
  int32_t crop[2];      /* the draw's crop: rows, columns */
  int32_t crop_offset;  /* of the draw's crop in the packed crops, in pixels of one section */
  int32_t reserved;     /* 0; the struct is 64 bytes */
} bsmi_aug2d_draw;
int bsmi_aug2d_coords(int device, const bsmi_aug2d_draw *draws, const bsmi_aug2d_draw *draws_dev, int S, int K, const int64_t input_shape[2],
                      const int64_t frame_offset[2], const int64_t frame_shape[2], const int32_t *shifts_dev, const float *lattice_dev,
                      int64_t lattice_floats, float *coords_dev, void *stream);
int bsmi_aug2d_sample_f32_u8(int device, const bsmi_aug2d_draw *draws, const bsmi_aug2d_draw *draws_dev, int S, int K, const float *coords_dev,
                             const int64_t frame_shape[2], const int64_t region_offset[2], const int64_t region_shape[2],
                             const uint8_t *crops_dev, int64_t crop_pixels, float *out_dev, void *stream);
int bsmi_aug2d_sample_nearest_i64(int device, const bsmi_aug2d_draw *draws, const bsmi_aug2d_draw *draws_dev, int S, int K,
                                  const float *coords_dev, const int64_t frame_shape[2], const int64_t region_offset[2],
                                  const int64_t region_shape[2], const int64_t *crops_dev, int64_t crop_pixels, int64_t *out_dev, void *stream);
int bsmi_aug2d_sample_nearest_u8(int device, const bsmi_aug2d_draw *draws, const bsmi_aug2d_draw *draws_dev, int S, int K,
                                 const float *coords_dev, const int64_t frame_shape[2], const int64_t region_offset[2],
                                 const int64_t region_shape[2], const uint8_t *crops_dev, int64_t crop_pixels, uint8_t *out_dev, void *stream);

/* ---- training augmentation of the 2-D setups: the intensity chain of raw, a whole batch per launch
 * (csrc/augment2d_intensity.hip; reference models/2d_mtlsd/train.py:123-136 and its 2d_affs / 2d_lsd siblings: NoiseAugment ->
 * IntensityAugment -> GammaAugment -> ImpulseNoiseAugment -> SmoothAugment -> DefectAugment under gp.Stack(10); the rules in
 * full: DESIGN.md sections 7k and 7m, tests/aug2d_intensity_ref.py) ----
 * The rule for draw s is the rule of the per-block chain above for the block (K, H, W) made of its K sections, unchanged --
 * the same device code (csrc/augment_intensity.h), so the results are the same bits: the Philox counter is the voxel's
 * linear index inside the draw's own stack, (k * H + y) * W + x; smoothing runs over all three axes of the stack, "reflect"
 * across the K sections.  The batch x_dev is the trainer's float32 [K][S][H][W], changed in place: the sections of a draw
 * are S planes apart.  Plane p = k * S + s; the per-plane tables scale_dev / shift_dev / gamma_dev (float32) and mode_dev
 * (int32) have K * S entries, and stats_dev is bsmi_aug_section_stats_f32 of the batch taken as K * S sections (the planes
 * are contiguous).  Each entry is ONE launch for all draws (smooth: two), grid.y over the planes, lanes along x; a draw
 * whose bit for the node is clear is left bit-equal, and a call in which no draw has the node launches nothing.
 *
 *   sample_unit_f32_u8   aug2d_sample_f32_u8 with the table: a draw with BSMI_AUG2D_TOUCHED is written v / 255 (one rounded
 *              division, the chain's input), every other draw exactly as aug2d_sample_f32_u8 writes it.
 *   noise      sigma and seed of the draw.           impulse    seed and impulse_threshold (<= 2^32) of the draw.
 *   intensity, gamma   the per-plane tables; rows of draws without the node are not read.
 *   smooth     the draw's 2 * radius + 1 normalised taps at taps_offset floats inside taps_dev (taps_floats long); z pass
 *              x_dev -> tmp_dev (a workspace of the batch's size; only the planes of smoothed draws are written and read),
 *              then the LDS-tiled y/x pass back.
 *   defect     mode per plane (`mode` in host memory is checked: 0 .. 3) for draws with BSMI_AUG2D_DEFECT; if final_map, then
 *              x = 2 x - 1 for every draw with BSMI_AUG2D_TOUCHED.  The contrast scale is the draw's.
 * The table is passed twice, as for the geometric chain: `idraws` in host memory, which every call checks (S < 1, K < 1,
 * more than 65535 planes, bits outside the mask, a radius above BSMI_AUG_MAX_RADIUS, taps beyond taps_floats, a threshold
 * above 2^32, K * S * H * W >= 2^31: BSMI_ERR_INVALID, nothing launched), and `idraws_dev`, the same bytes in device
 * memory, which the kernels read. */
#define BSMI_AUG2D_NOISE 1
#define BSMI_AUG2D_INTENSITY 2
#define BSMI_AUG2D_GAMMA 4
#define BSMI_AUG2D_IMPULSE 8
#define BSMI_AUG2D_SMOOTH 16
#define BSMI_AUG2D_DEFECT 32
#define BSMI_AUG2D_TOUCHED 64 /* some node changes the draw: resampled as v / 255, mapped 2 x - 1 at the end */
typedef struct bsmi_aug2d_idraw {
  uint64_t seed;              /* Philox key of noise and impulse */
  uint64_t impulse_threshold; /* floor(q * 2^32) */
  float noise_sigma;
  float contrast_scale;
  int32_t nodes;              /* mask of BSMI_AUG2D_* */
  int32_t radius;             /* of the smoothing taps, 0 .. BSMI_AUG_MAX_RADIUS */
  int32_t taps_offset;        /* of the draw's 2 * radius + 1 floats in the packed taps */
  int32_t reserved[3];        /* 0; the struct is 48 bytes */
} bsmi_aug2d_idraw;
int bsmi_aug2d_sample_unit_f32_u8(int device, const bsmi_aug2d_draw *draws, const bsmi_aug2d_draw *draws_dev, const bsmi_aug2d_idraw *idraws,
                                  const bsmi_aug2d_idraw *idraws_dev, int S, int K, const float *coords_dev, const int64_t frame_shape[2],
                                  const int64_t region_offset[2], const int64_t region_shape[2], const uint8_t *crops_dev, int64_t crop_pixels,
                                  float *out_dev, void *stream);
int bsmi_aug2d_noise_f32(int device, const bsmi_aug2d_idraw *idraws, const bsmi_aug2d_idraw *idraws_dev, int S, int K, const int64_t shape[2],
                         float *x_dev, void *stream);
int bsmi_aug2d_intensity_f32(int device, const bsmi_aug2d_idraw *idraws, const bsmi_aug2d_idraw *idraws_dev, int S, int K,
                             const int64_t shape[2], float *x_dev, const float *stats_dev, const float *scale_dev, const float *shift_dev,
                             void *stream);
int bsmi_aug2d_gamma_f32(int device, const bsmi_aug2d_idraw *idraws, const bsmi_aug2d_idraw *idraws_dev, int S, int K, const int64_t shape[2],
                         float *x_dev, const float *stats_dev, const float *gamma_dev, void *stream);
int bsmi_aug2d_impulse_f32(int device, const bsmi_aug2d_idraw *idraws, const bsmi_aug2d_idraw *idraws_dev, int S, int K, const int64_t shape[2],
                           float *x_dev, void *stream);
int bsmi_aug2d_smooth_f32(int device, const bsmi_aug2d_idraw *idraws, const bsmi_aug2d_idraw *idraws_dev, int S, int K, const int64_t shape[2],
                          float *x_dev, float *tmp_dev, const float *taps_dev, int64_t taps_floats, void *stream);
int bsmi_aug2d_defect_f32(int device, const bsmi_aug2d_idraw *idraws, const bsmi_aug2d_idraw *idraws_dev, int S, int K, const int64_t shape[2],
                          float *x_dev, const float *stats_dev, const int32_t *mode, const int32_t *mode_dev, int final_map, void *stream);

/* ---- training augmentation of the second-stage inputs (csrc/augment_inputs.hip; reference models/3d_affs_from_2d_mtlsd/
 * train.py:110-126 and its three siblings, "simulate noisy defected predictions": NoiseAugment -> IntensityAugment per channel
 * -> IntensityAugment per section -> SmoothAugment per section -> DefectAugment (low contrast only); the rules in full:
 * DESIGN.md section 7n, tests/augin_ref.py) ----
 * Specified rules, like the chains above: parity with gunpowder is in distribution.  One input array is a float32
 * x_dev [C][D][H][W] with values in [0, 1], changed in place; channels are axis 0, sections (the z planes) axis 1, and plane
 * p = c * D + z is H * W contiguous floats.  Each node is one call; a node the caller's plan skips is simply not called.
 * Stateless, asynchronous on `stream`; fewer than 2^31 voxels, at most 65535 planes (BSMI_ERR_INVALID otherwise).  The
 * per-voxel arithmetic is that of the intensity chain of raw (csrc/augment_intensity.h), the same device code.
 *
 *   noise      bsmi_aug_noise_f32 on the array taken as [C * D][H][W]: the Philox counter is the linear index within the
 *              array, ((c * D + z) * H + y) * W + x, so every channel has its own noise.  No entry of its own.
 *   group_mean mean_dev [C] (axis 0: of every channel over its D, H, W) or [D] (axis 1: of every section over C, H, W).
 *              Deterministic, no atomics: the sum of every plane is taken as bsmi_aug_section_stats_f32 takes it on
 *              [C * D][H][W] (BSMI_AUG_STAT_PARTS fixed chunks in a fixed order, combined in index order) and divided by
 *              H * W; a group's mean then adds the means of its planes in index order (z = 0 .. D - 1 of the channel, c = 0 ..
 *              C - 1 of the section) and divides by their number.  workspace_dev: BSMI_AUGIN_WORKSPACE_FLOATS(C, D) floats.
 *   intensity  x = clip(m_g + (x - m_g) * scale_g + shift_g, 0, 1), g the voxel's channel (axis 0) or section (axis 1);
 *              mean_dev, scale_dev, shift_dev: float32 [C] or [D].
 *   smooth     per section z a separable Gaussian with the section's own normalised taps, weights_dev [D][2 *
 *              BSMI_AUG_MAX_RADIUS + 1] float32 (the first 2 * radius_dev[z] + 1 of a row are read) and radius_dev [D] int32,
 *              border "reflect" (d c b a | a b c d, repeated where the radius exceeds the axis); passes along c (x_dev ->
 *              tmp_dev, a workspace of the array's size; a thread holds its column's C values, C <= BSMI_AUGIN_MAX_CHANNELS),
 *              then y and x (one launch, from a tile staged with its halo in LDS, tmp_dev -> x_dev); each tap sum runs from
 *              tap 0 upwards, and the last one is held to [0, 1], which the exact sum never leaves (the float32 taps can add
 *              up to 1 and a few ulp).  channels = 0 makes the c pass a copy.  A section of radius 0 is touched by neither launch; the
 *              kernels hold a radius to 0 .. BSMI_AUG_MAX_RADIUS, so no table takes them beyond their tiles.
 *   contrast   mode_dev int32 [D]: a section of mode 3 becomes x = m_z + (x - m_z) * contrast_scale with m_z = mean_dev[z]
 *              (group_mean, axis 1); every other section is not touched. */
#define BSMI_AUGIN_MAX_CHANNELS 16
#define BSMI_AUGIN_WORKSPACE_FLOATS(C, D) ((size_t)(C) * (D) * (BSMI_AUG_STAT_PARTS * 3 + 3))
int bsmi_augin_group_mean_f32(int device, const int64_t shape[4], const float *x_dev, float *workspace_dev, int axis, float *mean_dev,
                              void *stream);
int bsmi_augin_intensity_f32(int device, const int64_t shape[4], float *x_dev, const float *mean_dev, const float *scale_dev,
                             const float *shift_dev, int axis, void *stream);
int bsmi_augin_smooth_f32(int device, const int64_t shape[4], float *x_dev, float *tmp_dev, const float *weights_dev, const int32_t *radius_dev,
                          int channels, void *stream);
int bsmi_augin_contrast_f32(int device, const int64_t shape[4], float *x_dev, const float *mean_dev, const int32_t *mode_dev,
                            float contrast_scale, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BSMI_H */
