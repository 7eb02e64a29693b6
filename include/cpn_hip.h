/* libcpn_hip.so -- C ABI of the MI355X (gfx950) Contour Proposal Network inference path.
 *
 * The reference (FZJ-INM1-BDA/celldetection v0.4.9) is pure Python: the "FFI" this library replaces is the set of
 * PyTorch / torchvision operator calls on the CPN inference path.  Each entry point cites the reference call
 * site(s) it replaces (paths relative to the reference repository root).  The Python binding a maintainer would
 * add is a ctypes stub (see INTEGRATION.md and celldetection_amd/_lib.py).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types.  All device pointers are HIP device memory owned by the
 *     caller (e.g. PyTorch's caching allocator); the library allocates no device memory after plan creation
 *     except what the caller hands it as workspace.
 *   - every call enqueues on the caller's HIP stream (`stream` = hipStream_t cast to void*), no internal threads,
 *     no host synchronisation unless stated.
 *   - return value: 0 = ok, otherwise a negative CPN_E_* code or a positive hipError_t; cpn_last_error() returns a
 *     thread-local message.  No exceptions cross the ABI.
 */
#ifndef CPN_HIP_H
#define CPN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPN_ABI_VERSION 22

#define CPN_E_INVALID (-1)
#define CPN_E_UNSUPPORTED (-2)
#define CPN_E_WORKSPACE (-3)
#define CPN_E_INTERNAL (-4) /* a bound that holds by construction was reached (ABI 20: the contour trace) */

#define CPN_HOST /* the pointer is to host memory; an array parameter (`int32_t info[5]`) always is and carries no mark */

const char *cpn_last_error(void);
int cpn_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * Conv-graph plan: the backbone + head convolution stack.
 * Replaces CPNCore.forward (celldetection/models/cpn.py:238-283): backbone(inputs) [models/unet.py:296-304,178-249;
 * models/fpn.py:180-185; models/resnet.py:265-297 + torchvision block forwards], the four ReadOut heads
 * (models/commons.py:461-511) and Normalize's range assert (models/commons.py:694-700).
 * ---------------------------------------------------------------------------------------------------------- */

/* activation tensors of the graph (NHWC bf16, channel count padded to a multiple of 32) */
typedef struct {
    int32_t channels;  /* padded channel count (multiple of 32; 64 for CPN_PRECISION_FP8 plans)   */
    int32_t down;      /* nominal down-sampling factor (1,2,4,...,32); actual sizes are propagated per input size */
    float scale;       /* CPN_PRECISION_FP8: value of one e4m3 code unit of this tensor (> 0); a NEGATIVE scale marks a tensor
                        * stored as bf16 values inside an fp8 plan -- the partial sums between the PHASE and the LATERAL op of
                        * a sub-pixel triple (ABI 11).  Other precisions: unused */
} cpn_tensor_desc;

/* CPN_OP_CONV_DEFERRED (score-gated heads, cpn_sparse_heads below): a fused ReadOut head conv that cpn_plan_run does NOT
 * execute -- its weights are packed and its output size is reported like a CPN_OP_CONV's, and its source tensor stays
 * intact in the workspace until the end of the run (cpn_plan_tensor_info locates it). */
/* CPN_OP_INPUT_STEM / CPN_OP_STEM7 (bf16 and fp8 plans; csrc/stem.hip): the ResNet stem `body.0` = Conv2d(in_channels <= 4 -> 32 | 64
 * output channels after padding, 7x7, stride 2, pad 3) + BN + ReLU (celldetection/models/resnet.py:274-284) on a dedicated
 * layout: CPN_OP_INPUT_STEM converts the input to bf16 [N][H + 6][W + 8][4] with a zero border inside the storage of its
 * dst tensor (which needs (H + 6) * (W + 8) * 4 <= H * W * channels elements), CPN_OP_STEM7 reads it with weights
 * [7][cout_b][32] bf16 at weight_offset (filter row, output channel, (kx 0..7, c 0..3); kx = 7 and c >= in_channels zero).
 * Both carry `alt` = 2 and stand next to the generic CPN_OP_INPUT / CPN_OP_CONV pair (`alt` = 1): the executor runs the
 * fast pair at every input size the layout fits into the tensor, the generic pair otherwise. */
/* CPN_OP_CONV_PAIR (bf16 plans; csrc/conv_pair.hip): the head of a grouped bottleneck block -- conv1 1x1 + BN + ReLU ->
 * conv2 3x3 (groups, stride 1 | 2, pad 1) + BN + ReLU, torchvision Bottleneck.forward as built by
 * celldetection/models/resnet.py:88-116,119-193 for the ResNeXt encoders -- as ONE kernel: conv1's output stays in LDS.
 * The op stands directly BEHIND the two CPN_OP_CONV ops it restates (conv1 at index i - 2, conv2 at i - 1) and adds no
 * weights: src0 = conv1's source, dst = conv2's destination, cin_b / cout_b = conv1's input / output channels,
 * weight_offset / bias_offset = conv1's, fuse_weight_offset / fuse_bias_offset = conv2's, bundles = conv2's bundles,
 * fuse_cout = conv2's channels per bundle (32 | 64).  The executor runs it INSTEAD of the two convs at every input size at
 * which the kernel applies -- feature maps exactly 16 | 32 | 64 pixels wide as full-width row strips (conv1 output channels
 * a multiple of 256; 128 at width 64), any other width > 32 as generic 16 x 32 tiles (multiple of 128, 32-channel bundles);
 * a stride-2 conv2 (`stride` = 2: the first block of a stage) on generic tiles at any width >= 32 -- and batch x tiles x
 * slabs give >= 192 workgroups; the two convs run otherwise.  Same operands and per-conv
 * rounding (bf16 activations between the two convs) as the unfused pair; conv1 is recomputed on one halo row above and
 * below each 8-row strip. */
/* CPN_OP_CONV_BRIDGE (bf16 plans, ABI 11; csrc/conv_igemm.hip MODE_BR): the bridge level of the ResNet-UNets -- TwoConvNormRelu
 * (bias-free convs, celldetection/models/unet.py:92-107; commons.py:120-149) over the x2 nearest-upsampled 64-channel map
 * (unet.py:213-217, `scale_factor=2`) -- as ONE kernel: the first conv runs as its CPN_SUBPIXEL_SCATTER form (four 2x2 phase convs
 * + bias + ReLU) on the halo tile of the second conv's workgroup and lands in LDS, the full-resolution tensor between the two
 * convs is neither written nor read.  The op stands directly BEHIND the two CPN_OP_CONV ops it restates (the SCATTER conv at
 * index i - 2, the 3x3 conv at i - 1) and adds no weights: src0 = the scatter conv's source (32 | 64 channels), dst / res /
 * res_up / act = the 3x3 conv's, cin_b = the scatter conv's input channels, cout_b = 64, weight_offset / bias_offset = the
 * scatter conv's, fuse_weight_offset / fuse_bias_offset = the 3x3 conv's.  The executor runs it INSTEAD of the two convs
 * wherever the output is at least 16 x 32 pixels and nothing else reads the tensor in between (CPN_BRIDGE=0 in the
 * environment: never); same operands, K order and rounding points as the two launches. */
enum { CPN_OP_INPUT = 0, CPN_OP_CONV = 1, CPN_OP_MAXPOOL = 2, CPN_OP_BILINEAR = 3, CPN_OP_CONV_DEFERRED = 4,
       CPN_OP_INPUT_STEM = 5, CPN_OP_STEM7 = 6, CPN_OP_CONV_PAIR = 7, CPN_OP_CONV_BRIDGE = 8, CPN_OP_ACT = 9 };
/* 4..12 (ABI 11): hidden activations of the ReadOut heads other than ReLU (`head_activation*`, celldetection/models/cpn.py:183-233), as
 * the torch.nn modules of those names compute them with default arguments.  They are ops of their own -- CPN_OP_ACT: dst = act(src0),
 * elementwise on an NHWC tensor of any precision -- between the head's k x k conv (act NONE, not fused) and its 1x1 conv; conv ops
 * take CPN_ACT_NONE .. CPN_ACT_TANH_SCALED only */
enum { CPN_ACT_NONE = 0, CPN_ACT_RELU = 1, CPN_ACT_SIGMOID = 2, CPN_ACT_TANH_SCALED = 3, CPN_ACT_LEAKY_RELU = 4, CPN_ACT_SILU = 5,
       CPN_ACT_GELU = 6, CPN_ACT_ELU = 7, CPN_ACT_TANH = 8, CPN_ACT_HARDSWISH = 9, CPN_ACT_MISH = 10, CPN_ACT_SELU = 11,
       CPN_ACT_SOFTPLUS = 12 };
/* Sub-pixel decomposition of a k = 3 conv over cat(lateral, nearest-x2-upsampled top-down map) -- the first conv of every
 * GeneralizedUNet decoder level (celldetection/models/unet.py:213-224).  Output pixel (2i+py, 2j+px) sees the upsampled
 * map through 2 x 2 distinct low-resolution pixels only, so that part of the conv is FOUR 2 x 2 convs on the
 * low-resolution map (4/9 of the multiply-accumulates, tap sums rounded to bf16 once).  In a plan such a conv is a
 * triple of consecutive ops:
 *   CPN_SUBPIXEL_HEAD     the conv as the reference states it (virtual concat + nearest resize in the loader)
 *   CPN_SUBPIXEL_PHASE    src0 = top-down map, kh = kw = 2, `bundles` = 4 output phases (py, px) that all read the SAME
 *                         cin_b input channels with padding (pad - py, pad - px); dst = [h/2, w/2, 4 * cout_b] partial
 *                         sums (no bias, no activation), phase-major channels
 *   CPN_SUBPIXEL_LATERAL  src0 = lateral, res = the phase tensor read pixel-shuffled (res_up = 2), bias + activation,
 *                         dst = the HEAD op's dst
 * The executor runs PHASE + LATERAL when the lateral is exactly twice the top-down map's size and HEAD otherwise
 * (any other ratio: PyTorch's nearest index does not decompose).
 *   CPN_SUBPIXEL_SCATTER  a k = 3 conv whose ONLY source is a x2-upsampled map (`scale_factor=2`: always exact; the
 *                         bridge levels of GeneralizedUNet, unet.py:100-107,213-217) as a single op: the four 2 x 2 phase
 *                         convs (kh = kw = 2, bundles = 4 sharing cin_b input channels and ONE bias of cout_b entries)
 *                         + bias + activation, each phase written to its pixels (2i+py, 2j+px) of the [2h, 2w, cout_b]
 *                         destination.  Replaces the conv it restates (no HEAD op).
 * Bilinear counterpart -- the k x k ReadOut conv over the x2 BILINEAR-resized feature map in front of the FPN models'
 * refinement head (celldetection/models/cpn.py:277-278 + commons.py:461-511; fused ReadOut heads with k = 3 (mod 4), i.e.
 * 3 or the default 7).  For an exact x2 the resized map is a fixed linear filter of the low-resolution map (up[2i] =
 * .25 x[i-1] + .75 x[i], up[2i+1] = .75 x[i] + .25 x[i+1] per axis), so the conv is FOUR k2 x k2 convs on the low-resolution
 * map, k2 = (k + 3) / 2 (25 instead of 49 taps per output pixel for k = 7; tap sums formed in float64, rounded to bf16
 * once) -- wherever the conv window does not reach beyond the resized image.  A triple of consecutive ops again:
 *   CPN_SUBPIXEL_BL_HEAD   the conv as the reference states it (bf16 plans: up0 == 2, bilinear resize in the loader; fp8
 *                          plans: up0 == 0, src0 = the output of a CPN_OP_BILINEAR op of its own)
 *   CPN_SUBPIXEL_BL_PHASE  src0 = the low-resolution map (no resize; fp8 plans: the map in FRONT of that resize op), kh = kw =
 *                          k2, pad = k2 / 2, `bundles` = 4 output
 *                          phases sharing cin_b input channels, ONE bias and the fused tail; phase (py, px) writes pixel
 *                          (2i + py, 2j + px) of the external output for the low-resolution pixels i in [F/2, h - F/2)
 *   CPN_SUBPIXEL_BL_FRAME  the HEAD op restricted to the frame of F full-resolution pixels along every edge (F = 4 for
 *                          k = 7, 2 for k = 3), where the conv's zero padding cuts the window
 *                          (launched on the tiles that reach into the frame only; per tile row that crosses the interior ONE
 *                          wrap tile = output columns W - 16 .. W - 1 and 0 .. 15).  A CPN_OP_BILINEAR op flagged
 *                          CPN_SUBPIXEL_BL_FRAME feeds such a triple: when PHASE + FRAME run it writes only the ring of its
 *                          output the frame's windows reach (F + k / 2 pixels from the border)
 * The executor runs PHASE + FRAME when the input is exactly twice the feature map's size and the tile-granular frame leaves
 * a gain (CPN_BLPHASE=0 / 2 in the environment: never / wherever exact), HEAD otherwise. */
enum { CPN_SUBPIXEL_NONE = 0, CPN_SUBPIXEL_HEAD = 1, CPN_SUBPIXEL_PHASE = 2, CPN_SUBPIXEL_LATERAL = 3,
       CPN_SUBPIXEL_SCATTER = 4, CPN_SUBPIXEL_BL_HEAD = 5, CPN_SUBPIXEL_BL_PHASE = 6, CPN_SUBPIXEL_BL_FRAME = 7 };
enum { CPN_OUT_SCORES = 0, CPN_OUT_LOCATIONS = 1, CPN_OUT_FOURIER = 2, CPN_OUT_REFINEMENT = 3, CPN_OUT_UNCERTAINTY = 4,
       CPN_NUM_OUTPUTS = 5 };

typedef struct {
    int32_t op;               /* CPN_OP_*                                                                   */
    int32_t src0, src1, res;  /* tensor ids (-1 = none). src1: second source of a virtual channel concat      */
    int32_t dst;              /* tensor id, or -1 when the op writes an external fp32 NCHW output             */
    int32_t up0, up1, res_up; /* 1: source / residual is nearest-resized (PyTorch 'nearest': floor(dst*in/out)) to the
                               * size of the other concat source / of the output; a lone up0 source: exact x2.
                               * res_up == 2: the residual is a CPN_SUBPIXEL_PHASE tensor [h/2, w/2, 4 * C] read
                               * pixel-shuffled: out(y, x, c) += res(y >> 1, x >> 1, ((y & 1) * 2 + (x & 1)) * C + c).
                               * up0 == 2: src0 is read through a BILINEAR resize (align_corners=False) to the input
                               * size H x W (cpn.py:277-278; k x k stride-1 single-source convs of bf16 / fp8 plans) */
    int32_t c0_used;          /* channels of the concat taken from src0 (multiple of 32)                      */
    int32_t kh, kw, stride, pad;
    int32_t bundles, cin_b, cout_b; /* grouped convs run as `bundles` dense convs of cin_b -> cout_b channels  */
    int64_t weight_offset;    /* byte offset into the packed weight blob: [bundle][(cin_b/32)*kh*kw items, + one
                               * all-zero item when that count is odd][cout_b][32] bf16 (chunk-major, tap-minor)  */
    int64_t bias_offset;      /* float offset into the bias blob, -1 = no bias                                 */
    int32_t act;              /* CPN_ACT_*                                                                    */
    float act_scale;
    int32_t out_index;        /* dst == -1: CPN_OUT_* index of the external output                            */
    int32_t cout_real;        /* dst == -1: real number of output channels                                    */
    int32_t dst_coff;         /* channel offset inside dst                                                    */
    int32_t in_channels;      /* CPN_OP_INPUT: real input channels                                            */
    /* fused ReadOut tail (dst == -1 and fuse_cout > 0): conv -> act -> bf16 -> 1x1 conv [32][cout_b] bf16 at
     * fuse_weight_offset (+ fuse_bias_offset, -1 = none) -> fuse_act -> fp32 NCHW output `out_index` with fuse_cout
     * channels; requires bundles == 1 and cout_b in {32, 64, 128, 256} */
    int64_t fuse_weight_offset, fuse_bias_offset;
    int32_t fuse_cout, fuse_act;
    float fuse_act_scale;
    int32_t mult_offset;      /* CPN_PRECISION_FP8: float offset into the bias blob of the per-output-channel
                               * multipliers (weight scales), -1 = none; unused by the other precisions        */
    int32_t subpixel;         /* CPN_SUBPIXEL_* (bf16 plans)                                                    */
    int32_t alt;              /* 0: always runs; 1 / 2: generic / fast member of the stem alternatives (see above)  */
} cpn_op_desc;

typedef struct cpn_plan cpn_plan;

/* precision of a plan: bf16 activations/weights on MFMA with fp32 accumulation (the performance path), or an fp32
 * verification path (fp32 activations/weights/FMA on the vector ALUs; weights packed [bundle][kh*kw][cin_b][cout_b]
 * fp32, weight_offset in bytes of that blob; no fused heads) used to check the whole path against the reference's
 * fp32 CPU forward at 1e-4 */
enum { CPN_PRECISION_BF16 = 0, CPN_PRECISION_F32 = 1, CPN_PRECISION_FP8 = 2 };
/* CPN_PRECISION_FP8 (groundwork for BASELINE.json configs[4], no reference counterpart): activations are OCP e4m3
 * codes with one static scale per tensor (cpn_tensor_desc.scale, taken from a bf16 run through cpn_plan_run_stats),
 * weights e4m3 codes with one scale per output channel and the input-tensor scale folded in (see cpn_conv2d_fp8),
 * accumulation in fp32 on v_mfma_scale_f32_32x32x64_f8f6f4 (2x the bf16 MFMA rate); the fused ReadOut tails stay
 * bf16, the head outputs fp32. */

/* Creates a plan (host-side object; copies the descriptors).  `weights` / `bias` are DEVICE pointers to the packed
 * blobs and must stay alive as long as the plan. */
int cpn_plan_create(cpn_plan **plan, const cpn_tensor_desc *tensors, int32_t n_tensors, const cpn_op_desc *ops,
                    int32_t n_ops, const void *weights, size_t weight_bytes, const float *bias, size_t bias_count,
                    int32_t precision);
void cpn_plan_destroy(cpn_plan *plan);
/* Workspace (activation arena, liveness-planned) needed for a batch of N inputs of H x W.  Any H, W the graph can
 * digest: tensor sizes are propagated op by op with the reference modules' rules (conv / max-pool floor((in+2p-k)/s)+1;
 * top-down maps nearest-resized to the lateral's size, models/unet.py:213-217 and torchvision FPN; features
 * bilinear-resized to the input size, models/cpn.py:277-278); too small an input returns CPN_E_INVALID. */
int64_t cpn_plan_workspace_bytes(cpn_plan *plan, int32_t N, int32_t H, int32_t W);
/* Spatial size (h, w) of the external output CPN_OUT_* for an H x W input (0 x 0: the plan has no such output), and
 * the element count per image of the largest activation tensor (callers split batches at 2^31 elements). */
int cpn_plan_output_dims(cpn_plan *plan, int32_t H, int32_t W, int32_t out_index, CPN_HOST int32_t *h, CPN_HOST int32_t *w);
int64_t cpn_plan_max_tensor_elements(cpn_plan *plan, int32_t H, int32_t W);
/* Location of activation tensor `tensor` inside the workspace of a (N, H, W) run: byte offset, spatial size and channel
 * stride (padded channel count; NHWC, bf16 / e4m3 / fp32 by plan precision).  Only tensors that are live at the end of the
 * run may be read afterwards -- the sources of CPN_OP_CONV_DEFERRED ops are. */
int cpn_plan_tensor_info(cpn_plan *plan, int32_t N, int32_t H, int32_t W, int32_t tensor, CPN_HOST int64_t *byte_offset,
                         CPN_HOST int32_t *h, CPN_HOST int32_t *w, CPN_HOST int32_t *channel_stride);
/* 2*MAC FLOPs executed by the MFMA loops for that shape (includes channel/tile padding). */
double cpn_plan_executed_flops(cpn_plan *plan, int32_t N, int32_t H, int32_t W);

/* Runs the conv graph.  input: fp32 (dtype 0) or uint8 (dtype 1, scaled by 1/255) NCHW [N,C,H,W].
 * outputs[CPN_OUT_*] (CPN_NUM_OUTPUTS pointers; unused ones may be NULL): fp32 NCHW device buffers: scores
 * [N,1,h,w] with the sigmoid applied (binary) or raw logits [N,classes,h,w] (multi-class, cpn.py:583-585), locations
 * [N,2,h,w], fourier [N,4*order,h,w], refinement [N,2*buckets,H,W] (tanh*margin applied), uncertainty [N,4,h,w]
 * (sigmoid applied; only for plans with an uncertainty head, cpn.py:209-221).
 * range_flag: device int32, zeroed by the caller; set to 1 if an input value lies outside [0,1]
 * (the caller raises the reference's AssertionError, models/commons.py:696-697). */
int cpn_plan_run(cpn_plan *plan, const void *input, int32_t in_dtype, int32_t N, int32_t H, int32_t W,
                 void *workspace, int64_t workspace_bytes, float *const *outputs, int32_t *range_flag, void *stream);

/* Calibration run of a CPN_PRECISION_BF16 plan: like cpn_plan_run, additionally writes max|x| of every activation
 * tensor to absmax[tensor id] (device float[n_tensors], zeroed by the caller). */
int cpn_plan_run_stats(cpn_plan *plan, const void *input, int32_t in_dtype, int32_t N, int32_t H, int32_t W,
                       void *workspace, int64_t workspace_bytes, float *const *outputs, int32_t *range_flag,
                       float *absmax, void *stream);

/* Profiling variant: brackets every op with HIP events on `stream`, synchronises, and returns the per-op duration
 * (ms, op_ms[cpn_plan_num_ops]) and the executed MFMA FLOPs per op (op_flops, may be NULL). */
int cpn_plan_num_ops(cpn_plan *plan);
int cpn_plan_run_timed(cpn_plan *plan, const void *input, int32_t in_dtype, int32_t N, int32_t H, int32_t W,
                       void *workspace, int64_t workspace_bytes, float *const *outputs, int32_t *range_flag,
                       void *stream, CPN_HOST float *op_ms, CPN_HOST double *op_flops);

/* Single convolution (testing / building blocks); same semantics as one CPN_OP_CONV. */
int cpn_conv2d(const cpn_op_desc *op, const void *src0, int32_t c0_stride, const void *src1, int32_t c1_stride,
               const void *res, int32_t res_stride, void *dst, int32_t dst_stride, int32_t N, int32_t Hin, int32_t Win,
               const void *weights, const float *bias, void *stream);
/* fp8 (OCP e4m3) variant of cpn_conv2d on v_mfma_scale_f32_32x32x64_f8f6f4 (BASELINE.json configs[4] groundwork; no
 * reference counterpart): activations and residual are e4m3 codes (NHWC, channel strides multiples of 64, value =
 * code * tensor scale), weights are e4m3 codes packed [bundle][cin/64][kh*kw (+1 zero slab when the item count is
 * odd)][cout][64] with the input-tensor scale folded in before quantisation; value = acc * mult[cout] + bias
 * (+ residual code * res_scale) -> act -> e4m3(value * out_inv_scale) (NHWC outputs) or the fp32 head outputs. */
int cpn_conv2d_fp8(const cpn_op_desc *op, const void *src0, int32_t c0_stride, const void *src1, int32_t c1_stride,
                   const void *res, int32_t res_stride, void *dst, int32_t dst_stride, int32_t N, int32_t Hin,
                   int32_t Win, const void *weights, const float *bias, const float *mult, float res_scale,
                   float out_inv_scale, void *stream);
/* ResNet stem fast path (see CPN_OP_INPUT_STEM / CPN_OP_STEM7): input conversion into the padded 4-channel layout
 * (dst: (H + 6) * (W + 8) * 4 bf16 per image) and the 7x7 stride-2 conv + bias + ReLU from it (`op`: a CPN_OP_STEM7
 * descriptor; dst NHWC bf16 [N][(H - 1) / 2 + 1][(W - 1) / 2 + 1][dst_stride], or -- out_inv_scale > 0, the output tensor
 * of an fp8 plan -- OCP e4m3 codes of value * out_inv_scale; the stem computes in bf16 on the bf16 input either way). */
int cpn_convert_input_stem(const void *src, int32_t in_dtype, void *dst, int32_t N, int32_t C, int32_t H, int32_t W,
                           int32_t *range_flag, void *stream);
int cpn_stem7(const cpn_op_desc *op, const void *src, void *dst, int32_t dst_stride, int32_t N, int32_t H, int32_t W,
              const void *weights, const float *bias, float out_inv_scale, void *stream);
/* Fused bottleneck head (see CPN_OP_CONV_PAIR; `op`: such a descriptor, `weights` / `bias`: the blobs its four offsets
 * index): src NHWC bf16 [N][H][W][c_stride] -> dst NHWC bf16 [N][Ho][Wo][dst_stride], channels [0, cout_b), Ho = (H - 1) /
 * op->stride + 1.  Returns
 * CPN_E_UNSUPPORTED when W < 16 or between 17 and 31, or cout_b is no multiple of the slab width (run the two convs). */
int cpn_conv_pair(const cpn_op_desc *op, const void *src, int32_t c_stride, void *dst, int32_t dst_stride, int32_t N,
                  int32_t H, int32_t W, const void *weights, const float *bias, void *stream);
/* Fused bridge level (see CPN_OP_CONV_BRIDGE; `op`: such a descriptor, `weights` / `bias`: the blobs its four offsets point
 * into): src = [N, H, W, c_stride] bf16 low-resolution map, dst = [N, 2H, 2W, dst_stride] bf16; res (optional) = a residual of
 * the 3x3 conv at the output's size.  CPN_E_UNSUPPORTED when the kernel's shape does not apply (output below 16 x 32 pixels). */
int cpn_conv_bridge(const cpn_op_desc *op, const void *src, int32_t c_stride, const void *res, int32_t res_stride, void *dst,
                    int32_t dst_stride, int32_t N, int32_t H, int32_t W, const void *weights, const float *bias, void *stream);
/* Which kernel would run (ABI 18): the instantiation conv_igemm_kernel<TH, BN, WM, WN, mode> that cpn_conv2d (precision =
 * CPN_PRECISION_BF16; a CPN_OP_CONV_BRIDGE descriptor: cpn_conv_bridge with c0_stride = its c_stride and Hin x Win = its
 * H x W) or cpn_conv2d_fp8 (CPN_PRECISION_FP8) launches for the same descriptor, strides and sizes -> info = {mode
 * (CPN_CONV_MODE_*), TH (tile rows), BN (output channels per block), WM, WN (wave grid)}; a tile is TH x 32 pixels (MODE_N:
 * 2 TH rows of a 16-column output).  A second source / a residual is present iff op->src1 >= 0 / op->res >= 0.  Runs the
 * argument building, validation and tile selection of the launch itself and returns what the launch returns for a call it
 * rejects, but makes no HIP call and touches no buffer: it answers on a machine without a GPU.  The CPN_S1F / CPN_S1Q
 * environment switches are read per call, as by the launch. */
#define CPN_CONV_MODE_PW 0   /* 1x1, pad 0                                   */
#define CPN_CONV_MODE_S1 1   /* k x k, stride 1                              */
#define CPN_CONV_MODE_S2 2   /* k x k, stride 2                              */
#define CPN_CONV_MODE_BL 3   /* k x k over a bilinear-resized source (bf16)  */
#define CPN_CONV_MODE_N 6    /* outputs 16 columns wide (bf16)               */
#define CPN_CONV_MODE_S1F 7  /* two workgroups per CU, <8,128,4,2> (bf16)    */
#define CPN_CONV_MODE_BR 8   /* fused bridge level, <16,64,2,2> (bf16)       */
#define CPN_CONV_MODE_S1Q 10 /* four K items per step, <16,64,2,2> (bf16)    */
int cpn_conv2d_kernel_info(const cpn_op_desc *op, int32_t precision, int32_t c0_stride, int32_t c1_stride, int32_t res_stride,
                           int32_t dst_stride, int32_t N, int32_t Hin, int32_t Win, int32_t info[5]);
int cpn_maxpool2d(const void *src, void *dst, int32_t N, int32_t Hin, int32_t Win, int32_t C, int32_t k, int32_t stride,
                  int32_t pad, void *stream);
int cpn_resize_bilinear(const void *src, void *dst, int32_t N, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout,
                        int32_t C, void *stream);
int cpn_convert_input(const void *src, int32_t in_dtype, void *dst, int32_t N, int32_t C, int32_t H, int32_t W,
                      int32_t Cpad, int32_t *range_flag, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Proposal extraction + contour decode.
 * ---------------------------------------------------------------------------------------------------------- */

/* Order-preserving stream compaction of (scores > thresh), replaces `torch.where(fg_mask)`
 * (celldetection/models/cpn.py:579,616-620): writes the linear indices (b*h*w + y*w + x, ascending = (b,y,x)
 * row-major order) of the selected pixels to `indices` (capacity N*h*w int32) and the per-image counts to
 * `counts` (N+1 int32: counts[b] = proposals of image b, counts[N] = total).  `workspace`: cpn_compact_workspace_bytes. */
int64_t cpn_compact_workspace_bytes(int32_t N, int32_t h, int32_t w);
int cpn_compact(const float *scores, int32_t N, int32_t h, int32_t w, float thresh, int32_t *indices, int32_t *counts,
                void *workspace, void *stream);

/* Fused gather + rel->abs location + Fourier-to-contour synthesis + rescale + local refinement + clamp + boxes
 * (+ per-image offsets).  Replaces celldetection/models/cpn.py:613-702 i.e. rel_location2abs_location
 * (ops/cpn.py:15-41), advanced-index gathers (cpn.py:621-628), fouriers2contours (ops/cpn.py:44-95), scale_contours /
 * scale_fourier (ops/cpn.py:106-165), local_refinement (cpn.py:63-85), clamp + min/max boxes (cpn.py:661-670) and the
 * offsets add (cpn.py:695-702).
 *   indices[P]           from cpn_compact
 *   scores [N,1,h,w], locations [N,2,h,w], fourier [N,4*order_total,h,w], refinement [N,2,H,W] or NULL (fp32 NCHW)
 *   order <= order_total (cpn.py:597-598 "changed order"), samples = S, iterations = refinement iterations
 *   cos_table/sin_table [order][samples] fp32 device (built by the host exactly like ops/cpn.py:69-78)
 *   offsets: float [N,2] (xy) device or NULL (the reference adds int64 offsets to fp32 tensors = fp32 add of the
 *   converted value); when no refinement runs, contours and contour_proposals are ONE tensor in the reference and
 *   receive the offset twice (cpn.py:655-656,697-699) -- reproduced
 *   buckets = refinement_buckets (cpn.py:72-82): 1 = plain map; > 1: refinement is [N,2*buckets,H,W] and
 *   bucket_index / bucket_weight are [3][samples] device tables (bucket number and blend weight of the three
 *   neighbouring buckets of every sample, built by the host like resolve_refinement_buckets, ops/cpn.py:238-255)
 * outputs (device, row-major): contours [P,S,2], proposals [P,S,2], boxes [P,4], out_scores [P], out_locations [P,2],
 *   out_fourier [P,order,4], batch_index [P] int32. */
int cpn_decode(const int32_t *indices, int32_t P, const float *scores, const float *locations, const float *fourier,
               const float *refinement, int32_t N, int32_t h, int32_t w, int32_t H, int32_t W, int32_t order_total,
               int32_t order, int32_t samples, int32_t iterations, const float *cos_table, const float *sin_table,
               const float *offsets, float *contours, float *proposals, float *boxes, float *out_scores,
               float *out_locations, float *out_fourier, int32_t *batch_index, int32_t buckets,
               const int32_t *bucket_index, const float *bucket_weight, void *stream);

/* cpn_decode on GATHERED head values: locations [P,2] and fourier [P,4*order_total] hold the head outputs of proposal p
 * (what cpn_sparse_heads writes) instead of dense maps; everything else as cpn_decode. */
int cpn_decode_gathered(const int32_t *indices, int32_t P, const float *scores, const float *locations,
                        const float *fourier, const float *refinement, int32_t N, int32_t h, int32_t w, int32_t H,
                        int32_t W, int32_t order_total, int32_t order, int32_t samples, int32_t iterations,
                        const float *cos_table, const float *sin_table, const float *offsets, float *contours,
                        float *proposals, float *boxes, float *out_scores, float *out_locations, float *out_fourier,
                        int32_t *batch_index, int32_t buckets, const int32_t *bucket_index, const float *bucket_weight,
                        void *stream);

/* Score-gated ReadOut heads (bf16 plans): evaluates two fused ReadOut heads (cpn_op_desc with fuse_cout > 0: k x k
 * stride-1 'same' conv + BN + ReLU + 1x1 conv, celldetection/models/commons.py:461-511) that read the same NHWC bf16
 * feature tensor [N,h,w,channel_stride] ONLY at the P pixels `indices` (cpn_compact's output) and writes out_a [P,
 * op_a->fuse_cout] and out_b [P, op_b->fuse_cout] (fp32): bit-identical to the values the dense heads produce at those
 * pixels.  CPN.forward reads the location / Fourier maps at the proposals only (celldetection/models/cpn.py:613-637); the
 * dense maps are (N h w) / P times more work.  `weights` / `bias`: the plan's packed blobs (the ops' offsets index them).
 * Both heads must share source, kernel size and hidden width (128 or 256). */
int cpn_sparse_heads(const cpn_op_desc *op_a, const cpn_op_desc *op_b, const void *features, int32_t channel_stride,
                     int32_t N, int32_t h, int32_t w, const int32_t *indices, int32_t P, const void *weights,
                     const float *bias, float *out_a, float *out_b, void *stream);

/* Standalone pieces of the decode (parity tests, reference ops API celldetection/ops/cpn.py). */
int cpn_fouriers2contours(const float *fourier, const float *locations, int32_t P, int32_t order, int32_t samples,
                          const float *cos_table, const float *sin_table, float *contours, void *stream);
int cpn_local_refinement(float *contours /* in/out [P,S,2] */, const int32_t *batch_index, int32_t P, int32_t samples,
                         const float *refinement, int32_t N, int32_t H, int32_t W, int32_t iterations,
                         int32_t buckets, const int32_t *bucket_index, const float *bucket_weight, void *stream);

/* Score variants of CPN.forward.
 * cpn_class_scores (multi-class CPNs, celldetection/models/cpn.py:583-585,631-632): softmax over the C logit planes
 * [N,C,h,w], optional score bounds lower/upper [N,1,h,w] applied to every class plane (_apply_score_bounds,
 * cpn.py:118-123), classes = argmax (first maximum), selected = probability of that class, foreground = 1.0 where
 * classes > 0 else 0.0 (feeds cpn_compact with thresh 0.5).  probs [N,C,h,w] may be NULL.
 * cpn_certainty_mask (cpn.py:617-618): out = scores where mean_c(uncertainty[N,C,h,w]) < limit, else -1
 * (limit = 1 - certainty_thresh), so that the thresholding in cpn_compact applies `fg_mask &= ...`.
 * cpn_gather_channels (cpn.py:634-636): out[p][c] = map[b][c][y][x] for the pixel index indices[p] of cpn_compact. */
int cpn_class_scores(const float *logits, int32_t N, int32_t C, int32_t h, int32_t w, const float *lower,
                     const float *upper, float *probs, float *selected, int32_t *classes, float *foreground,
                     void *stream);
int cpn_certainty_mask(const float *scores, const float *uncertainty, int32_t N, int32_t C, int32_t h, int32_t w,
                       float limit, float *out, void *stream);
int cpn_gather_channels(const float *map, const int32_t *indices, int64_t P, int32_t C, int32_t h, int32_t w,
                        float *out, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Box NMS.  Replaces torch.ops.torchvision.nms as called from batched_box_nmsi (celldetection/ops/cpn.py:189-227)
 * and the slide-level NMS (celldetection_scripts/cpn_inference.py:405-408,426): greedy, stable descending-score
 * order, suppress iff inter/(area_i+area_j-inter) > thresh (NaN never suppresses), output = kept indices in that
 * order.  Segmented: boxes/scores hold `nseg` consecutive segments (images) [seg_offsets[s], seg_offsets[s+1]);
 * segments are independent.  seg_offsets_host: host int64[nseg+1]; seg_offsets_dev: same values on the device.
 * keep (int64 [P], device): for each segment the kept indices (GLOBAL indices into boxes/scores, i.e. segment start
 * + index within the segment; descending score) are written from position seg_offsets[s]; keep_counts
 * (int32 [nseg], device) receives the number kept per segment.
 * ---------------------------------------------------------------------------------------------------------- */
int64_t cpn_nms_workspace_bytes(int64_t P, int64_t max_segment, int32_t nseg);
int cpn_nms(const float *boxes, const float *scores, int64_t P, CPN_HOST const int64_t *seg_offsets_host,
            const int64_t *seg_offsets_dev, int32_t nseg, float thresh, int64_t *keep, int32_t *keep_counts,
            void *workspace, int64_t workspace_bytes, void *stream);

/* Box voting of the multi-model ensemble path (get_iou_voting / filter_by_box_voting, celldetection/ops/boxes.py:52-83,
 * called from celldetection_scripts/cpn_inference.py:419-423): votes[i] = sum_j iou(i,j) * (iou(i,j) > thresh), IoU
 * as torchvision.ops.box_iou; every box votes for itself (smallest vote 1).  boxes [P,4] fp32 (16-byte aligned). */
int cpn_box_votes(const float *boxes, int64_t P, float thresh, float *votes, void *stream);

/* remove_border_contours (celldetection/ops/cpn.py:258-290): keep[i] = 1 iff all points of contour i (+offset)
 * satisfy y>pad (top), x<w-pad (right), y<h-pad (bottom), x>pad (left) on the enabled sides.
 * sides: bit0 top, bit1 right, bit2 bottom, bit3 left. */
int cpn_border_keep(const float *contours, int64_t P, int32_t samples, float off_x, float off_y, float h, float w,
                    float pad, int32_t sides, uint8_t *keep, void *stream);

/* F.interpolate(x, size, mode='bilinear', align_corners=False) on fp32 NCHW planes: `_equal_size` of the score-bound
 * masks and head maps (celldetection/models/cpn.py:109-123,279).  src [planes, Hin, Win] -> dst [planes, Hout, Wout]. */
int cpn_resize_bilinear_f32(const float *src, float *dst, int64_t planes, int32_t Hin, int32_t Win, int32_t Hout,
                            int32_t Wout, void *stream);
/* The same with the mode of CPNCore's `refinement_interpolation` (celldetection/models/cpn.py:109-115,277-279): mode 0 =
 * bilinear (= cpn_resize_bilinear_f32), 1 = bicubic (PyTorch's cubic convolution, A = -0.75, align_corners=False).  The
 * non-interpolating modes cannot run in the reference (torch rejects align_corners for them) and are no modes here.
 * Inside a plan the resize op CPN_OP_BILINEAR selects bicubic with act = 1 (bf16 / fp32 plans). */
int cpn_resize_f32(const float *src, float *dst, int64_t planes, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout,
                   int32_t mode, void *stream);

/* Measurement aid (no reference counterpart): shader clock of the bf16 implicit-GEMM conv kernels, measured inside the kernels.
 * Only libcpn_hip_clock.so (csrc/conv_igemm.hip compiled with -DCPN_EXP_CLOCK=2; built next to libcpn_hip.so, selected with
 * CPN_HIP_LIB) carries the probe: one workgroup of every conv launch adds the s_memtime ticks (shader clock) and the 100-MHz
 * s_memrealtime ticks its main loop took, its K steps, 1, and 4 x the matrix-pipe cycles its MFMAs occupy per SIMD (all waves of the
 * CU counted) to out15[5 * bin + 0..4], bin 0 = 7x7 convs, 1 = 3x3, 2 = other tap counts.  out15 (host, may be NULL) receives the
 * sums, reset != 0 clears them afterwards.  The product library returns 1 ("built without the clock probe").  bench.py reports
 * shader MHz = 100 * ticks / ref ticks and matrix-pipe duty = pipe cycles / ticks next to the roofline. */
int cpn_debug_clock_probe(CPN_HOST unsigned long long *out15, int reset);

/* The same rule for ALL detections of a forwarded batch of tiles in one launch (the per-tile loop of
 * celldetection_scripts/cpn_inference.py:370-380): contour p belongs to image image_index[p] (int32, device);
 * sides[n] (int32, device) is the bit mask above of tile n, offsets[n] = (x, y) floats ADDED to the coordinates
 * (the reference passes -tile_offset); h, w, pad as above. */
int cpn_border_keep_batched(const float *contours, int64_t P, int32_t samples, const int32_t *image_index,
                            const int32_t *sides, const float *offsets, int32_t n_images, float h, float w, float pad,
                            uint8_t *keep, void *stream);

/* Slide-scale NMS: same semantics and the SAME keep list as cpn_nms with one segment (torchvision nms: greedy, stable
 * descending-score order), computed with a spatial grid + sparse suppressor lists + a monotone fixed point instead of
 * the dense P x P/64 bit mask -- O(P + E) memory, E = number of (box, higher-ranked box with IoU > thresh) pairs.
 * Replaces the global NMS over all detections of a slide (celldetection_scripts/cpn_inference.py:405-408,426).
 * Needs thresh >= 0.  max_edges: capacity of the caller's edge buffer; when E exceeds it the call returns
 * CPN_E_WORKSPACE with *edges_needed = E (retry with a larger workspace).  keep: int64 [P] device (first
 * *keep_count_host entries valid); keep_count_dev (optional) receives the count on the device as well.
 * sweeps (optional, host): number of fixed-point sweeps executed.  This call SYNCHRONISES the stream (it reads E, the
 * convergence counter and the keep count back). */
int64_t cpn_nms_binned_workspace_bytes(int64_t P, int64_t max_edges);
int cpn_nms_binned(const float *boxes, const float *scores, int64_t P, float thresh, int64_t max_edges, int64_t *keep,
                   int64_t *keep_count_dev, CPN_HOST int64_t *keep_count_host, CPN_HOST int64_t *edges_needed, CPN_HOST int32_t *sweeps,
                   void *workspace, int64_t workspace_bytes, void *stream);

/* Slide preprocessing before tiling: `preprocess` -> cd.data.normalize_percentile
 * (celldetection_scripts/cpn_inference.py:196-222, celldetection/data/misc.py:156-161).
 * cpn_histogram: value histogram of an 8-bit (dtype 1, 256 bins) or 16-bit (dtype 2, 65536 bins) image into the
 * pre-zeroed uint32 array `hist` (the caller derives np.percentile's interpolated order statistics from it).
 * cpn_rescale_to_uint8: out = uint8(rint(((clip(x, low, high) - low) / (high - low)) * 255)) in float64
 * (normalize_percentile + skimage.img_as_ubyte); x: dtype 0 = f32, 1 = u8, 2 = u16. */
int cpn_histogram(const void *x, int32_t dtype, int64_t n, uint32_t *hist, void *stream);
int cpn_rescale_to_uint8(const void *x, int32_t dtype, int64_t n, double low, double high, uint8_t *out, void *stream);

/* Tile pre-filter of the slide loop.  Replaces the per-tile `mask[slices].any()` of TileLoader
 * (celldetection_scripts/cpn_inference.py:88-100: tiles whose mask / point-mask crop is empty are skipped): for every
 * window i = (y0, y1, x0, x1) of `windows` (int32 [n][4], device; bounds inside the H x W map -- the caller's tiling
 * table) out[i] |= any(mask[y0:y1, x0:x1] != 0).  mask: [H][W] row-major, dtype 0 = f32, 1 = u8 / bool; out: int32 [n]
 * device, pre-zeroed by the caller.  ONE launch and no host synchronisation for the whole table. */
int cpn_window_any(const void *mask, int32_t dtype, int32_t H, int32_t W, const int32_t *windows, int32_t n, int32_t *out,
                   void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Label rasterisation.  Replaces celldetection.data.contours2labels / render_contour
 * (celldetection/data/cpn.py:245-255,292-358; called from celldetection_scripts/cpn_inference.py:811):
 * contour k is rounded (half to even), clipped to the image, filled as a polygon (OpenCV
 * drawContours(thickness=-1) rule for integer vertices, restated) and added with value k + 1 to the FIRST channel whose
 * region [bbox expanded by `gap`] holds no label yet.  The sequential loop of the reference is resolved in rounds over
 * mutually independent contours (see csrc/labels.hip); the caller drives the rounds:
 *   cpn_labels_prepare:     contours fp32 [K,S,2] -> integer points [K,S,2], boxes [K,4] = (xmin, ymin, xmax, ymax)
 *   cpn_labels_bin:         cell id of every box centre for a grid_w x grid_h grid of `cell`-pixel cells (cell >= largest
 *                           box extent + gap + 1) and the identity index; the caller sorts (stably) by cell id
 *   cpn_labels_cell_bounds: [begin, end) of every non-empty cell in the sorted order (arrays pre-zeroed)
 *   cpn_labels_round:       ONE round: marks the contours whose predecessors are all painted, chooses their channel on
 *                           the planar int32 canvas [channels][H][W] and paints them.  counters_host[0] = painted in
 *                           this round, [1] = contours that found all `channels` occupied (grow the canvas, call
 *                           again), [2] = ready contours.  Synchronises the stream.  use_ioa != 0 (`ioa_thresh`,
 *                           data/cpn.py:341-350): a ready contour whose filled area is covered by labels of any channel
 *                           to more than ioa_thresh (int / int in float64, like numpy) is resolved WITHOUT painting:
 *                           state = 2, counted in counters_host[0].  Painted contours carry the provisional value k + 1;
 *                           the caller renumbers to the reference's running label (k + 1 - skipped contours before k).
 * ---------------------------------------------------------------------------------------------------------- */
int cpn_labels_prepare(const float *contours, int64_t K, int32_t S, int32_t H, int32_t W, int32_t rounded, int32_t clip,
                       int32_t *points, int32_t *boxes, void *stream);
int cpn_labels_bin(const int32_t *boxes, int64_t K, int32_t grid_w, int32_t grid_h, int32_t cell, uint32_t *cell_id,
                   uint32_t *index, void *stream);
int cpn_labels_cell_bounds(const uint32_t *sorted_cell_id, int64_t K, uint32_t *cell_begin, uint32_t *cell_end,
                           void *stream);
int cpn_labels_round(const int32_t *points, const int32_t *boxes, int64_t K, int32_t S, int32_t H, int32_t W,
                     int32_t gap, int32_t grid_w, int32_t grid_h, int32_t cell, const uint32_t *sorted_index,
                     const uint32_t *cell_begin, const uint32_t *cell_end, int32_t *canvas, int32_t channels,
                     uint8_t *state, uint8_t *ready, uint32_t *ready_list, int32_t *channel, int32_t *counters,
                     CPN_HOST int32_t *counters_host, int32_t use_ioa, double ioa_thresh, void *stream);

/* ----------------------------------------------------------------------------------------------------------
 * Instance evaluation of label images (cd.data.LabelMatcher, celldetection/data/instance_eval.py; csrc/instance_eval.hip).
 * Label images: int32 [pixels][channels] on the device, channel-interleaved, 16-byte aligned; values <= 0 are background;
 * up to 8 channels per side (CPN_E_UNSUPPORTED above).
 *   workspace_bytes: bytes for a table of `table_capacity` slots (a power of two) plus the selection state of `pairs`
 *                    pairs over at most `labels` labels per side; pass 0 for the part a call does not use.
 *   pairs:           zeroes the table and counts, on the 64-bit key (input << 32 | target): the pixels of every distinct
 *                    (input label, target label) pair (a pixel counts once per pair), under (label << 32) the elements of
 *                    every input label and under (label) those of every target label.  Asynchronous.
 *   table_status:    status_host[0] = inserts that found no slot (> 0: repeat cpn_eval_pairs with a larger table),
 *                    [1] = occupied slots.  Synchronises the stream.  May be repeated: every call counts afresh.
 *   compact:         the occupied slots -> keys / counts (int64 [entries], device) in no particular order.
 *   unions:          for the pairs (sorted keys): position of both labels in the sorted label lists and
 *                    unions = input count + target count - intersection.  Synchronises the stream.
 *   select:          greedy one-to-one matching at iou_thresh: pairs with intersection / union (float64) >= iou_thresh, taken
 *                    from the largest IoU down (exact comparison i1 * u2 vs i2 * u1; equal IoU: lower pair position first)
 *                    unless one of their labels is taken.  selected: uint8 [pairs]; result_host[0] = pairs taken,
 *                    [1] = rounds.  Synchronises the stream.
 * ---------------------------------------------------------------------------------------------------------- */
int64_t cpn_eval_workspace_bytes(int64_t table_capacity, int64_t pairs, int64_t labels);
int cpn_eval_pairs(const int32_t *inputs, int32_t c_in, const int32_t *targets, int32_t c_t, int64_t pixels,
                   int64_t table_capacity, void *workspace, int64_t workspace_bytes, void *stream);
int cpn_eval_table_status(void *workspace, int64_t table_capacity, CPN_HOST int64_t *status_host, void *stream);
int cpn_eval_compact(void *workspace, int64_t table_capacity, int64_t *keys, int64_t *counts, int64_t entries, void *stream);
int cpn_eval_unions(const int64_t *pair_keys, const int64_t *intersections, int64_t pairs, const int64_t *input_labels,
                    const int64_t *input_counts, int64_t n_inputs, const int64_t *target_labels, const int64_t *target_counts,
                    int64_t n_targets, int64_t *unions, int32_t *input_index, int32_t *target_index, void *workspace,
                    void *stream);
int cpn_eval_select(const int64_t *intersections, const int64_t *unions, const int32_t *input_index, const int32_t *target_index,
                    int64_t pairs, int64_t n_inputs, int64_t n_targets, double iou_thresh, uint8_t *selected, void *workspace,
                    int64_t workspace_bytes, CPN_HOST int64_t *result_host, void *stream);

/* ----------------------------------------------------------------------------------------------------------
 * Flat label images (cd.data.resolve_label_channels, celldetection/data/cpn.py:361-399; called from
 * celldetection_scripts/cpn_inference.py:817; csrc/flat_labels.hip).  labels: int32 [H][W][channels] on the device,
 * channel-interleaved, 16-byte aligned; lbl: int32 [H][W], 16-byte aligned, the result.  A pixel with more than one
 * channel > 0 is an overlap pixel, with exactly one a core pixel.  H * W <= 2^31 - 1 (CPN_E_UNSUPPORTED above).
 * The propagation works on tiles of 32 x 32 pixels; one call of cpn_flat_step runs at most CPN_FLAT_MAX_STEPS steps.
 * All calls for one image use the same workspace.
 *   workspace_bytes: counters, a second [H][W] image and the tile flags.
 *   classify:        plain_max == 0: lbl = channel maximum at core pixels, -1 at overlap pixels (unresolved), 0 elsewhere;
 *                    marks the tiles that hold overlap pixels.  plain_max != 0: lbl = channel maximum (the result of an
 *                    image without overlap pixels).  status_host[0] = overlap pixels, [1] = pixels whose maximum is
 *                    negative (they differ between the two modes).  Synchronises the stream, unless status_host is NULL.
 *   step:            `steps` (1 .. CPN_FLAT_MAX_STEPS) synchronous steps: every unresolved pixel takes the maximum of lbl over the
 *                    neighbours named by `footprint` (bit 3 * row + column of a 3 x 3 array anchored at its centre; 0272 is
 *                    the 4-neighbourhood of cv2.getStructuringElement(MORPH_CROSS, (3, 3))), all pixels at once from the
 *                    values of the previous step; neighbours outside the image take no part.  `launch` counts the calls for
 *                    this image from 0: only tiles with unresolved pixels next to a change of the previous call run.
 *                    status_host[0] = pixels that received a label, [1] = tiles run.  0 pixels: a fixed point.
 *                    Synchronises the stream, unless status_host is NULL.
 *   finish:          what is still unresolved becomes 0.  Asynchronous.
 * ---------------------------------------------------------------------------------------------------------- */
#define CPN_FLAT_MAX_STEPS 8
int64_t cpn_flat_workspace_bytes(int32_t H, int32_t W);
int cpn_flat_classify(const int32_t *labels, int32_t channels, int32_t H, int32_t W, int32_t plain_max, int32_t *lbl,
                      void *workspace, int64_t workspace_bytes, CPN_HOST int64_t *status_host, void *stream);
int cpn_flat_step(int32_t *lbl, int32_t H, int32_t W, int32_t steps, int32_t footprint, int32_t launch, void *workspace,
                  int64_t workspace_bytes, CPN_HOST int64_t *status_host, void *stream);
int cpn_flat_finish(int32_t *lbl, int32_t H, int32_t W, void *workspace, int64_t workspace_bytes, void *stream);

/* ----------------------------------------------------------------------------------------------------------
 * Region property tables of label images (cd.data.labels2property_table, celldetection/data/misc.py:320-347, i.e.
 * skimage.measure.regionprops_table per channel; called from celldetection_scripts/cpn_inference.py:824-837;
 * csrc/region_props.hip).  ABI 17.
 * labels: int32 [H][W][channels] on the device, channel-interleaved, 16-byte aligned, channels <= 11; every element v > 0
 * belongs to the row of (channel, v).  intensity: NULL or an integer image [H][W][intensity_channels] (<= 4 channels) of
 * dtype CPN_PROPS_U8 / _I16 / _I32.  H * W <= 2^31 - 1 and H, W <= 65536 (CPN_E_UNSUPPORTED above): every sum fits int64.
 * All accumulation is integer arithmetic, the table is bit-identical from run to run.
 *   workspace_bytes: counters, a table of `table_capacity` slots (a power of two, <= 2^28) and the sort buffer.
 *   columns:         number of columns the property list expands to (-1: bad list; host only).
 *   accumulate:      zeroes the table and reads the image(s) once: per key the pixel count, the sums of r, c, r^2, r * c,
 *                    c^2 over global pixel coordinates, the bounding box and per intensity channel sum, minimum and
 *                    maximum.  Asynchronous.
 *   table_status:    status_host[0] = inserts that found no slot (> 0: repeat accumulate with a larger table),
 *                    [1] = occupied slots = rows.  Synchronises the stream.  May be repeated: every call counts afresh.
 *   compact_sort:    orders the occupied slots by (channel, label) ascending inside the workspace.  Asynchronous.
 *   finalise:        out: int64 [out_columns][entries] on the device with out_columns = columns + 1: one row per column in
 *                    the order of the property list (vectors and matrices in row-major order, intensity properties one
 *                    column per intensity channel), float columns as the bit pattern of the fp64 value, and a last row with
 *                    the channel of each entry.  Asynchronous.
 * Definitions, with the bounding box r0, c0, r1, c1 (half-open), the spacing (sy, sx) = (spacing_row, spacing_col) and the
 * sums shifted to the corner of the box in integers (sr = sum r - n * r0, srr = sum r^2 - 2 * r0 * sum r + n * r0^2, ...),
 * every expression evaluated in fp64 as written, without contraction:
 *   area = n * (sy * sx); area_bbox = ((r1 - r0) * (c1 - c0)) * (sy * sx); extent = area / area_bbox;
 *   equivalent_diameter_area = sqrt(4 * area / pi); centroid = ((sum r / n) * sy, (sum c / n) * sx);
 *   centroid_local = ((sr / n) * sy, (sc / n) * sx);
 *   mu20 = (srr - sr * sr / n) * (sy * sy); mu02 = (scc - sc * sc / n) * (sx * sx); mu11 = (src - sr * sc / n) * (sy * sx);
 *   inertia_tensor = [[a, b], [b, c]], a = mu02 / n, b = -mu11 / n, c = mu20 / n;
 *   inertia_tensor_eigvals = (l1, l2): m = (a + c) / 2, d = (a - c) / 2, s = sqrt(d * d + b * b), l1 = m + s, l2 = max(m - s, 0);
 *   axis_major_length = 4 * sqrt(l1); axis_minor_length = 4 * sqrt(l2); eccentricity = l1 == 0 ? 0 : sqrt(1 - l2 / l1);
 *   orientation = a - c == 0 ? (b < 0 ? pi / 4 : -pi / 4) : 0.5 * atan2(-2 * b, c - a);
 *   intensity_mean = sum i / n; intensity_min, intensity_max.
 * ---------------------------------------------------------------------------------------------------------- */
#define CPN_PROP_LABEL 0
#define CPN_PROP_BBOX 1
#define CPN_PROP_NUM_PIXELS 2
#define CPN_PROP_AREA 3
#define CPN_PROP_AREA_BBOX 4
#define CPN_PROP_EXTENT 5
#define CPN_PROP_EQUIVALENT_DIAMETER_AREA 6
#define CPN_PROP_CENTROID 7
#define CPN_PROP_CENTROID_LOCAL 8
#define CPN_PROP_INERTIA_TENSOR 9
#define CPN_PROP_INERTIA_TENSOR_EIGVALS 10
#define CPN_PROP_AXIS_MAJOR_LENGTH 11
#define CPN_PROP_AXIS_MINOR_LENGTH 12
#define CPN_PROP_ECCENTRICITY 13
#define CPN_PROP_ORIENTATION 14
#define CPN_PROP_INTENSITY_MEAN 15
#define CPN_PROP_INTENSITY_MIN 16
#define CPN_PROP_INTENSITY_MAX 17
#define CPN_PROP_COUNT 18
#define CPN_PROPS_U8 0
#define CPN_PROPS_I16 1
#define CPN_PROPS_I32 2
int64_t cpn_props_workspace_bytes(int64_t table_capacity, int32_t intensity_channels);
int32_t cpn_props_columns(CPN_HOST const int32_t *properties, int32_t n_properties, int32_t intensity_channels);
int cpn_props_accumulate(const int32_t *labels, int32_t H, int32_t W, int32_t channels, const void *intensity,
                         int32_t intensity_channels, int32_t intensity_dtype, int64_t table_capacity, void *workspace,
                         int64_t workspace_bytes, void *stream);
int cpn_props_table_status(void *workspace, int64_t table_capacity, CPN_HOST int64_t *status_host, void *stream);
int cpn_props_compact_sort(void *workspace, int64_t table_capacity, int32_t intensity_channels, int64_t entries, void *stream);
int cpn_props_finalise(void *workspace, int64_t table_capacity, int32_t intensity_channels, int64_t entries,
                       CPN_HOST const int32_t *properties, int32_t n_properties, double spacing_row, double spacing_col, int64_t *out,
                       int64_t out_columns, void *stream);

/* ----------------------------------------------------------------------------------------------------------
 * Shape property tables of label images: perimeter, perimeter_crofton, euler_number, area_convex, solidity (the outline
 * properties of skimage.measure.regionprops_table, which cd.data.labels2property_table hands on; csrc/shape_props.hip,
 * csrc/hull_count.h).  Entry points added to ABI 22 (nothing that existed changed; a library without them fails to load by its
 * missing symbols).  scikit-image is third-party and not available to this project: the arithmetic is restated
 * here, and these definitions are the contract.
 * The calls run after cpn_props_accumulate / table_status / compact_sort on the same label image: props_workspace is that
 * workspace (read only here: keys, pixel counts, bounding boxes, sorted order), with its table_capacity, intensity_channels
 * and entries.  Rows are the rows of cpn_props_finalise.  All accumulation is integer arithmetic: bit-identical from run to
 * run.
 *   workspace_bytes:    the shape workspace for a table of `table_capacity` slots (0: bad capacity).
 *   columns:            number of columns of the property list (every property is one column; -1: bad list; host only).
 *   heights:            heights int64 [entries] on the device: the bounding-box height of every row's object.  Asynchronous.
 *   accumulate:         zeroes the shape workspace and reads the label image once: per object the three perimeter classes,
 *                       the four transition counts and the bit-quad sum.  With row_begin != NULL (int64 [entries + 1] on the
 *                       device: the exclusive scan of `heights`, total_rows at the end; the caller scans) also the column
 *                       extent of every row of every object into extents (uint32 [2][total_rows], zeroed here).  Asynchronous.
 *   hull_scratch_bytes: scratch of `hull` (host only).
 *   hull:               counts int64 [entries] on the device: the lattice points of every object's convex hull, one lane per
 *                       object (an object as tall as the image serialises).  Asynchronous.
 *   finalise:           out: int64 [out_columns][entries] as cpn_props_finalise writes it (float columns as fp64 bit patterns,
 *                       a last row with the channel).  hull_counts may be NULL without area_convex / solidity.  Asynchronous.
 * Definitions.  For one row (channel z, label l) let M(r, c) = [labels[r][c][z] == l], and 0 outside the image: the predicate
 * is SAME LABEL, not foreground; a neighbouring pixel of another label counts as outside (as cropping to the bounding box,
 * regionprops(...).image, does).  n = number of pixels.  (sy, sx) = (spacing_row, spacing_col); s = sy, and perimeter /
 * perimeter_crofton with sy != sx are CPN_E_UNSUPPORTED (isotropic spacings only, as in scikit-image).  Every float
 * expression is evaluated in fp64 as written, without contraction; sqrt(2.0) and pi are the fp64 values.
 *   perimeter (perimeter(image, 4)): B(p) = M(p) and at least one of p's four edge neighbours has M = 0.  For each p with
 *     B(p): o = the number of its 4 edge neighbours with B, d = the number of its 4 diagonal neighbours with B, code =
 *     1 + 2 o + 10 d.  n1 = #{code in 5, 7, 15, 17, 25, 27}, n2 = #{code in 21, 33}, n3 = #{code in 13, 23}; every other
 *     code adds nothing.  perimeter = ((double) n1 + (double) n2 * sqrt(2.0) + (double) n3 * ((1.0 + sqrt(2.0)) / 2.0)) * s.
 *   perimeter_crofton (perimeter_crofton(image, 4)), as one-sided transition counts: Nv = #{M(r, c) and not M(r - 1, c)},
 *     Nh = #{M(r, c) and not M(r, c + 1)}, Nd = #{M(r, c) and not M(r - 1, c - 1)}, Na = #{M(r, c) and not M(r + 1, c - 1)};
 *     perimeter_crofton = (((double) (Nv + Nh) + (double) (Nd + Na) / sqrt(2.0)) * (pi / 4.0)) * s.
 *   euler_number (int64, ignores the spacing): 8-connected components of M minus 4-connected holes = (Q1 - Q3 - 2 QD) / 4 over
 *     all 2 x 2 windows of the zero-padded mask, (H + 1) x (W + 1) positions: Q1 / Q3 windows with one / three set pixels,
 *     QD windows with exactly the two diagonal pixels set.
 *   area_convex, solidity (convex_hull_image with offset_coordinates=True, include_borders=True): K = the closed convex hull
 *     of the points (r +- 1/2, c) and (r, c +- 1/2) over all pixels of M; cnt = the number of integer points (r, c) in K,
 *     decided with 64-bit integer cross products in doubled coordinates; area_convex = (double) cnt * (sy * sx);
 *     solidity = ((double) n * (sy * sx)) / area_convex.
 * ---------------------------------------------------------------------------------------------------------- */
#define CPN_SHAPE_LABEL 0
#define CPN_SHAPE_NUM_PIXELS 1
#define CPN_SHAPE_PERIMETER 2
#define CPN_SHAPE_PERIMETER_CROFTON 3
#define CPN_SHAPE_EULER_NUMBER 4
#define CPN_SHAPE_AREA_CONVEX 5
#define CPN_SHAPE_SOLIDITY 6
#define CPN_SHAPE_COUNT 7
int64_t cpn_shape_workspace_bytes(int64_t table_capacity);
int32_t cpn_shape_columns(CPN_HOST const int32_t *properties, int32_t n_properties);
int cpn_shape_heights(void *props_workspace, int64_t table_capacity, int32_t intensity_channels, int64_t entries, int64_t *heights,
                      void *stream);
int cpn_shape_accumulate(const int32_t *labels, int32_t H, int32_t W, int32_t channels, void *props_workspace, int64_t table_capacity,
                         int32_t intensity_channels, int64_t entries, void *workspace, int64_t workspace_bytes,
                         const int64_t *row_begin, uint32_t *extents, int64_t total_rows, void *stream);
int64_t cpn_shape_hull_scratch_bytes(int64_t entries, int64_t total_rows);
int cpn_shape_hull(int64_t entries, const int64_t *row_begin, const uint32_t *extents, int64_t total_rows, void *scratch,
                   int64_t scratch_bytes, int64_t *counts, void *stream);
int cpn_shape_finalise(void *props_workspace, int64_t table_capacity, int32_t intensity_channels, int64_t entries, void *workspace,
                       const int64_t *hull_counts, CPN_HOST const int32_t *properties, int32_t n_properties, double spacing_row,
                       double spacing_col, int64_t *out, int64_t out_columns, void *stream);

/* ----------------------------------------------------------------------------------------------------------
 * Overlay images (cd.data.contours2overlay, celldetection/data/cpn.py:647-662,699-723,811-855, and cd.label_cmap(ubyte=True),
 * celldetection/visualization/cmaps.py:21-77; both called from celldetection_scripts/cpn_inference.py:839-848;
 * csrc/overlay.hip).  ABI 19.  out: uint8 [H][W][4] (r, g, b, a) on the device, 4-byte aligned.  H * W <= 2^31 - 1
 * (CPN_E_UNSUPPORTED above).
 * contours2overlay: points int32 [K][S][2] and boxes int32 [K][4] are the outputs of cpn_labels_prepare (1 <= S <= 512),
 * colors uint8 [K][3].  Every contour is filled by the rule of the label rasteriser (csrc/polygon_fill.h); with n(p) contours
 * covering pixel p and S(p) the per-channel sum of their colours, out(p) = (Sr / n, Sg / n, Sb / n, 255) (integer division)
 * where n >= 1 and (0, 0, 0, 0) elsewhere.  The image is cut into tiles of CPN_OVERLAY_TILE x CPN_OVERLAY_TILE pixels,
 * tiles_x = ceil(W / tile), tiles = tiles_x * ceil(H / tile), tile index = ty * tiles_x + tx.  No full-image intermediate.
 *   bin_count: adds one to tile_count[t] (int32 [tiles], pre-zeroed) for every (contour, tile t its box meets).  Asynchronous.
 *   bin_fill:  tile_begin = int32 [tiles + 1], the exclusive scan of tile_count with the total (= pairs) at the end (the
 *              caller scans); cursor = int32 [tiles], pre-zeroed; writes the contour index of every pair into
 *              list[tile_begin[t] ..] (int32 [pairs]; the order within a tile is unspecified: the result does not depend on
 *              it).  Asynchronous.
 *   paint:     one workgroup per tile sums the colours of the contours of its list in LDS and writes every pixel of the
 *              image exactly once.  max_overlap: one device word, pre-zeroed, receives the largest n(p); with
 *              max_overlap_host != NULL it is copied there and the stream synchronised.  The sums are exact for
 *              n <= (2^32 - 1) / 255.  K = 0 (tile_begin all zero) writes zeros.
 * label_cmap: labels int32 [pixels][channels] on the device, channel-interleaved; table uint8 [rows][4] on the device,
 * 4-byte aligned, row 0 = the colour of label 0, rows >= 2.  Label v > 0 takes row v % (rows - 1) + 1.  reduce == 0 (channels
 * must be 1): out = the row.  reduce != 0: float32, in this order and without contraction: den = float(sum_c a_c) + 1e-12f;
 * for c = 0 .. channels - 1: w = a_c / den (correctly rounded), acc_j = acc_j + w * col_cj for j = r, g, b, a; out_j = acc_j
 * truncated.  flag: one device word, pre-zeroed, becomes non-zero when a label is negative (such pixels take row 0); with
 * flag_host != NULL it is copied there and the stream synchronised.
 * ---------------------------------------------------------------------------------------------------------- */
#define CPN_OVERLAY_TILE 32
int cpn_overlay_bin_count(const int32_t *boxes, int64_t K, int32_t H, int32_t W, int32_t *tile_count, void *stream);
int cpn_overlay_bin_fill(const int32_t *boxes, int64_t K, int32_t H, int32_t W, const int32_t *tile_begin, int32_t *cursor,
                         int32_t *list, int64_t pairs, void *stream);
int cpn_overlay_paint(const int32_t *points, const int32_t *boxes, const uint8_t *colors, int64_t K, int32_t S, int32_t H,
                      int32_t W, const int32_t *tile_begin, const int32_t *list, uint8_t *out, uint32_t *max_overlap,
                      CPN_HOST uint32_t *max_overlap_host, void *stream);
int cpn_label_cmap(const int32_t *labels, int64_t pixels, int32_t channels, int32_t reduce, const uint8_t *table, int32_t rows,
                   uint8_t *out, int32_t *flag, CPN_HOST int32_t *flag_host, void *stream);

/* ----------------------------------------------------------------------------------------------------------
 * Contours of label images (cd.data.labels2contours / labels2contour_list, celldetection/data/cpn.py:93-144, and
 * cd.data.resample_contours, celldetection/data/misc.py:371-405; csrc/label_contours.hip, csrc/components.h,
 * csrc/contour_trace.h).  ABI 20.
 * labels: int32 [H][W][channels] on the device, channel-interleaved, channels <= 65535, H * W <= 2^31 - 1 (CPN_E_UNSUPPORTED
 * above).  Rule: an object is a pair (channel, value v > 0); values <= 0 take no part.  Its components are the 8-connected sets
 * of pixels of that channel holding v.  An object with exactly one component yields one contour: Suzuki-Abe border following of
 * the outer border as cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE) does it -- start at the raster-first pixel (smallest y,
 * then smallest x); first search clockwise on screen from the west neighbour; every further search counter-clockwise, starting
 * after the pixel just left; every visit is a point (one-pixel-wide parts appear once per passage); stop when the start pixel
 * is re-entered from the first found neighbour; a single pixel gives its point twice; points are (x, y) in image coordinates.
 * An object with more than one component is fragmented and yields no contour.  Departure from cv2: a component that lies in a
 * hole of another component of the same value counts as a component.  Contours come by ascending value; of a value that is
 * unfragmented in several channels the highest such channel is returned.
 * All calls for one image use one workspace of cpn_contours_workspace_bytes(entries) bytes, entries >= the root count
 * (cpn_contours_workspace_bytes(0) suffices for cpn_contours_components), and the same roots image.
 *   components: roots = int32 [channels][H][W]: -1 where the value is <= 0, otherwise the index y * W + x of the raster-first
 *               pixel of the pixel's component (tiles of CPN_CONTOURS_TILE x CPN_CONTOURS_TILE pixels in LDS, then the seams with
 *               agent-scope atomics, then a flattening pass).  status_host[0] = components of all channels.  Synchronises.
 *   table:      entries = that count.  Replaces the word of every root in `roots` by -2 - (an internal slot); writes table =
 *               int32 [4][entries]: rows value, channel, root index, pixel count of the K contours to return, in their order
 *               (only the first K columns are written), and frag_values = int32 [entries]: the value of every component of a
 *               fragmented object, 0 elsewhere.  status_host[0] = K, [1] = components of fragmented objects.  Synchronises.
 *   count:      chan / root / npix = rows 1 .. 3 of the table.  One lane follows one border and counts its points: lengths =
 *               int64 [K], offsets = int64 [K + 1] (offsets[0] = 0, then the running sum).  status_host[0] = offsets[K] = all
 *               points.  A trace is capped at 8 * npix points (a pixel is entered from at most 8 directions); reaching the cap
 *               returns CPN_E_INTERNAL.  Synchronises.
 *   write:      the same traces again; points = int32 [offsets[K]][2] as (x, y).  A trace whose length differs from the counted
 *               one returns CPN_E_INTERNAL; no store goes beyond the contour's own range.  Synchronises.
 * resample_contours: points = double [total_points][2], contour k = points[offsets[k] .. offsets[k + 1]) with at least one
 * segment each (close != 0: the last point is joined to the first).  cumsum = double [total_points + K] scratch.  out = double
 * [K][num][2].  In fp64, in this order, without contraction: dt_i = sqrt(dx^2 + dy^2) + epsilon; cumsum = the running sum of
 * dt taken sequentially in index order; t_j = j * (cumsum_last / num); i = the first index with t_j <= cumsum_i; alpha =
 * (t_j - cumsum_(i-1)) / dt_i (cumsum_(-1) = 0); out_j = p_i * (1 - alpha) + p_(i+1) * alpha.  Asynchronous.
 * ---------------------------------------------------------------------------------------------------------- */
#define CPN_CONTOURS_TILE 32
int64_t cpn_contours_workspace_bytes(int64_t entries);
int cpn_contours_components(const int32_t *labels, int32_t channels, int32_t H, int32_t W, int32_t *roots, void *workspace,
                            int64_t workspace_bytes, CPN_HOST int64_t *status_host, void *stream);
int cpn_contours_table(const int32_t *labels, int32_t channels, int32_t H, int32_t W, int32_t *roots, int64_t entries,
                       int32_t *table, int32_t *frag_values, void *workspace, int64_t workspace_bytes, CPN_HOST int64_t *status_host,
                       void *stream);
int cpn_contours_count(const int32_t *roots, int32_t channels, int32_t H, int32_t W, int64_t K, const int32_t *chan,
                       const int32_t *root, const int32_t *npix, int64_t *lengths, int64_t *offsets, void *workspace,
                       int64_t workspace_bytes, CPN_HOST int64_t *status_host, void *stream);
int cpn_contours_write(const int32_t *roots, int32_t channels, int32_t H, int32_t W, int64_t K, const int32_t *chan,
                       const int32_t *root, const int32_t *npix, const int64_t *offsets, int32_t *points, void *workspace,
                       int64_t workspace_bytes, void *stream);
int cpn_resample_contours(const double *points, const int64_t *offsets, int64_t K, int64_t total_points, int32_t num,
                          int32_t close, double epsilon, double *cumsum, double *out, void *stream);

/* ----------------------------------------------------------------------------------------------------------
 * Elliptic Fourier descriptors of contours (cd.data.cpn.efd / contours2fourier, celldetection/data/cpn.py:23-90, 213-227;
 * csrc/contour_fourier.hip, csrc/efd_chunks.h).  ABI 21.
 * points: int32 or double [P][2] as (x, y) on the device (points_dtype = CPN_EFD_POINTS_*), read as they are; offsets: int64
 * [K + 1] on the device, contour k = points[offsets[k] .. offsets[k + 1]) with at least one point.  The call first checks on the
 * device that offsets starts at 0, ends at P and grows by at least one per contour, and returns CPN_E_INVALID otherwise; every
 * index into points, workspace and outputs is derived from offsets.  1 <= order <= CPN_EFD_MAX_ORDER.
 * Rule.  A contour of n points is closed if |first - last| <= 1e-8 + 1e-5 |last| holds for both coordinates (numpy's allclose
 * with b = last).  close_mode: CPN_EFD_CLOSE_NONE takes the contours as they are (N = n - 1 segments); the contours that are not
 * closed are counted in status_host[0], and when there is one nothing is computed (the caller raises).  CPN_EFD_CLOSE_ALL
 * appends the first point to every contour (N = n), CPN_EFD_CLOSE_EACH to the contours that are not closed.  For i = 0 .. N - 1:
 * dx_i, dy_i = the point differences, dt_i = sqrt(dx_i^2 + dy_i^2) + epsilon, t_0 = 0, t_(i+1) = t_i + dt_i, T = t_N.  For k = 1 ..
 * order with phi_(k,i) = k * (2 pi t_i / T) and C_k = T / (2 k^2 pi^2):
 *   coefficients[K][order][4]: C_k * (sum dx_i/dt_i dcos, sum dx_i/dt_i dsin, sum dy_i/dt_i dcos, sum dy_i/dt_i dsin) with
 *   dcos = cos phi_(k,i+1) - cos phi_(k,i), dsin likewise;
 *   locations[K][2]: first point + (a0, c0), a0 = (1/T) sum [dx_i/(2 dt_i) (t_(i+1)^2 - t_i^2) + (X_i - dx_i/dt_i t_(i+1)) dt_i],
 *   X_i = sum_(j<=i) dx_j (taken as x_(i+1) - x_0), c0 the same with y.
 * N = 0 (one point) gives coefficients 0 and location NaN; N = 1 with T = epsilon (the doubled point of labels2contours) gives
 * coefficients 0 and exactly that point.  All arithmetic is float64 without contraction.  Order of summation: a chunk is up to
 * CPN_EFD_CHUNK consecutive segments counted from the contour's own first segment; csrc/efd_chunks.h fixes the order within a
 * chunk and across chunks.  It depends on the contour alone: a result is bit-identical from run to run and wherever the
 * contour lies among others.  No floating-point atomics.
 * workspace: cpn_efd_workspace_bytes(K, P, order) bytes on the device (it grows with (P + K) / CPN_EFD_CHUNK * order: room for
 * the partial sums of contours of more than one chunk).  status_host: int64 [CPN_EFD_STATUS_WORDS] on the host: [0] contours
 * that are not closed, [1] chunks of contours of more than one chunk; with CPN_EFD_TIMED or-ed into close_mode [2 .. 6] are the
 * nanoseconds (HIP events) of: checks and work list, single-chunk contours, chunk sums and bases, partial sums, finish.
 * Synchronises (the checks are read back before anything else is launched).  K = 0 (P must be 0) does nothing.
 * ---------------------------------------------------------------------------------------------------------- */
#define CPN_EFD_CHUNK 256
#define CPN_EFD_MAX_ORDER 64
#define CPN_EFD_POINTS_I32 0
#define CPN_EFD_POINTS_F64 1
#define CPN_EFD_CLOSE_NONE 0
#define CPN_EFD_CLOSE_ALL 1
#define CPN_EFD_CLOSE_EACH 2
#define CPN_EFD_TIMED 256
#define CPN_EFD_STATUS_WORDS 8
int64_t cpn_efd_workspace_bytes(int64_t K, int64_t P, int32_t order);
int cpn_efd(const void *points, int32_t points_dtype, const int64_t *offsets, int64_t K, int64_t P, int32_t order, double epsilon,
            int32_t close_mode, void *workspace, int64_t workspace_bytes, double *coefficients_f64, double *locations_f64,
            CPN_HOST int64_t *status_host, void *stream);

/* ----------------------------------------------------------------------------------------------------------
 * CPN training targets (cd.data.labels2distances / mask_labels_by_distance_, celldetection/data/cpn.py:424-497, and
 * cd.data.filter_instances_, celldetection/data/segmentation.py:67-103; csrc/label_distances.hip).  ABI 22.
 * labels: int32 [H][W][channels] on the device, channel-interleaved; H, W <= 32768 (CPN_E_UNSUPPORTED above): every distance
 * fits uint32.  owner(p) = the one positive value at p when exactly one channel is > 0, otherwise 0.  distance_type selects the
 * weights of OpenCV's 3 x 3 chamfer transform in 16-bit fixed point (HV straight, DIAG diagonal): CPN_DIST_L2 (62587, 89738) =
 * round((0.955, 1.3693) * 2^16), CPN_DIST_L1 (1, 2) * 2^16, CPN_DIST_C (1, 1) * 2^16.  t(p) = min over zero pixels q of
 * DIAG * min(|dx|, |dy|) + HV * (max - min).  per_instance != 0: a zero pixel for p is every pixel whose owner differs from
 * owner(p), pixels outside the image included.  per_instance == 0: a zero pixel is a pixel with owner 0 inside the image.
 * All calls for one image use the same workspace, distance_type and per_instance.  Integer arithmetic until finalise, no
 * floating-point atomics: every result is bit-identical from run to run.
 *   workspace_bytes: counters, the owner image, two t images and the tile flags (0: H or W out of range).
 *   table_bytes:     the hash table (key, n, tmax) of `table_capacity` slots, a power of two from 64 to 2^28 (0 otherwise).
 *   classify:        owner and the seed of t (the cheapest step to an 8-neighbour that is a zero pixel; none: 2^32 - 1); marks
 *                    the 32 x 32 tiles that hold owner pixels.  status_host[0] = pixels with owner 0.  Synchronises the stream,
 *                    unless status_host is NULL.
 *   step:            `steps` (1 .. CPN_LABEL_DISTANCES_MAX_STEPS) synchronous steps t(p) = min(t(p), t(n) + w) over the
 *                    8-neighbours n that are no zero pixel for p, on every tile with owner pixels next to a change of the
 *                    previous call (`launch` counts the calls for this image from 0; call 0 runs all of them).
 *                    status_host[0] = pixels changed, [1] = tiles run.  0 pixels: the fixed point, t is final.
 *                    Synchronises the stream, unless status_host is NULL.
 *   reduce:          zeroes the table and accumulates per owner value n = pixel count and tmax = max t (per tile in LDS, then
 *                    one set of integer atomics per tile and value).  status_host[0] = inserts that found no slot (> 0: repeat
 *                    with a larger table).  Synchronises the stream, unless status_host is NULL.
 *   finalise:        distances float32 [H][W]: d = float32(t) * 2^-16; per_instance != 0: n > protected_size and tmax > 0:
 *                    d = d / (float32(tmax) * 2^-16); per_instance == 0: d = d / max(float32(tmax) * 2^-16, 1e-6f) (IEEE division,
 *                    no contraction); d clipped to [0, 1]; 0 where owner is 0.  labels_out int32 [H][W][channels] = labels with
 *                    every channel of an overlap pixel (more than one channel > 0) set to -1.  Asynchronous.
 *   mask:            in place on labels int32 [pixels][channels]: a pixel with any channel > 0 and d <= max_bg_dist gets all
 *                    channels 0; then a pixel with max_bg_dist < d < min_fg_dist gets all channels -1.  reduced: NULL or int32
 *                    [pixels], receives the channel maximum of the result.  Asynchronous.
 * cpn_label_remap: in place on int32 [elements]: an element equal to keys[i] (int32 [entries], ascending, distinct) becomes
 * values[i]; other elements stay.  One binary search per element.  Asynchronous.
 * ---------------------------------------------------------------------------------------------------------- */
#define CPN_LABEL_DISTANCES_MAX_STEPS 8
#define CPN_DIST_L1 1
#define CPN_DIST_L2 2
#define CPN_DIST_C 3
int64_t cpn_label_distances_workspace_bytes(int32_t H, int32_t W);
int64_t cpn_label_distances_table_bytes(int64_t table_capacity);
int cpn_label_distances_classify(const int32_t *labels, int32_t channels, int32_t H, int32_t W, int32_t distance_type,
                                 int32_t per_instance, void *workspace, int64_t workspace_bytes, CPN_HOST int64_t *status_host,
                                 void *stream);
int cpn_label_distances_step(int32_t H, int32_t W, int32_t steps, int32_t distance_type, int32_t per_instance, int32_t launch,
                             void *workspace, int64_t workspace_bytes, CPN_HOST int64_t *status_host, void *stream);
int cpn_label_distances_reduce(int32_t H, int32_t W, void *workspace, int64_t workspace_bytes, void *table,
                               int64_t table_capacity, CPN_HOST int64_t *status_host, void *stream);
int cpn_label_distances_finalise(const int32_t *labels, int32_t channels, int32_t H, int32_t W, int32_t per_instance,
                                 int32_t protected_size, void *workspace, int64_t workspace_bytes, const void *table,
                                 int64_t table_capacity, float *distances, int32_t *labels_out, void *stream);
int cpn_label_distances_mask(int32_t *labels, int32_t channels, int64_t pixels, const float *distances, float max_bg_dist,
                             float min_fg_dist, int32_t *reduced, void *stream);
int cpn_label_remap(int32_t *labels, int64_t elements, const int32_t *keys, const int32_t *values, int32_t entries, void *stream);

/* ----------------------------------------------------------------------------------------------------------
 * Training objective (the reference's CPN.forward(inputs, targets) in training mode, celldetection/models/cpn.py:561-692 with
 * compute_loss :441-559; csrc/cpn_objective.hip).  Additions to ABI 22.  This text is the contract.
 *
 * Inputs, all on the device.  Head maps, float32 NCHW: scores [N][score_channels][h][w] raw logits (1 channel: binary,
 * otherwise one per class), locations [N][2][h][w] relative (x, y), fourier [N][4 * order_total][h][w] of which the first
 * `order` coefficient rows are used, refinement [N][2 * buckets][H][W] or NULL.  Targets: labels [N][H][W] (int32, or int64 with
 * labels_i64 != 0), t_fourier [N][K][order][4], t_locations [N][K][2], t_contours [N][K][samples][2], t_classes int32 [N][K] or
 * NULL; cos_table / sin_table float32 [N][order][samples] of every image's own sampling (ops/cpn.py:66-78) and, with buckets > 1,
 * bucket_index int32 / bucket_weight float32 [N][3][samples] (ops/cpn.py:238-255), all four built by the caller with the
 * reference's expressions; order_weights float32 [order] or NULL (= 1).
 *
 * The rule.
 *  Labels go to the head grid by max pooling with kernel (H / h, W / w) (integer division, no padding) and, when the pooled
 *  size still differs from (h, w), by nearest interpolation (source index floor(i * float(in) / float(out)), at most in - 1).
 *  Foreground is > 0, background == 0; negative pixels are in neither set.
 *  Proposals are all foreground head pixels in (b, y, x) row-major order; proposal p takes the target row `label - 1` of its
 *  image b.  Its contour is decoded in float32 with the tables of image b exactly as cpn_decode does: ((location + pixel
 *  position) + sum of the sin terms) + sum of the cos terms, then times (float(W) / float(w), float(H) / float(h)); the
 *  selected coefficients and the absolute location are scaled after the decode.
 *  Refinement, `iterations` times: round half to even, clamp to the image, gather (three weighted buckets when buckets > 1),
 *  add -- as cpn_local_refinement.  Every refined set is clamped to [0, W - 1] x [0, H - 1] before it is used; without a
 *  refinement map or with iterations == 0 it is the proposals that are clamped.  A clamp passes a gradient where the value
 *  lay inside the closed range; nothing passes through the rounding.
 *  Box = minimum and maximum over the samples of the last set; on equal values the gradient goes to the lowest sample.
 *  Terms (n = number of elements; every |a - b| is a float32 difference, every sum float64 in an order fixed by the shapes):
 *   fourier    w_fourier * mean(|f * scale - t_fourier| * order_weights),         n = P * order * 4
 *   location   w_location * mean(|loc * scale - t_locations|),                    n = P * 2
 *   contour    w_contour * mean(|proposals - t_contours|),                        n = P * samples * 2
 *   refinement sum over the iterations of w_refinement * mean(|set - t_contours|)
 *   score      score_channels == 1: w_score_fg * mean over the foreground of BCE-with-logits(z, 1) + w_score_bg * mean over the
 *              background of BCE-with-logits(z, 0); otherwise cross entropy against t_classes[b][label - 1] (or 1) and 0.  A
 *              part whose set is empty is left out.  Elements are float64 functions of the float32 logits.
 *   iou        w_iou * mean of 1 - GIoU(box, target box) over the proposals whose box has float32 width and height >= 1; the
 *              target box is the minimum and maximum of the target contour; float64; no such proposal: 0.
 *  A mean that is not finite as float32 counts as 0 (add_to_loss_dict).  Every term is rounded to float32 once; the loss is
 *  the float32 sum of the terms that apply, in the order fourier, location, contour, score, refinement, boxes, iou, uncertainty.
 *  Gradients are the analytic derivatives of that loss in float64, rounded to float32 once per element (sign(0) = 0; equal
 *  arguments of a maximum or minimum of two boxes share the gradient evenly; clamp(min = 0) passes it on >= 0).
 *
 * The calls.
 *  cpn_objective_head (asynchronous): label pooling, foreground compaction (cpn_compact), the score elements and g_scores.
 *   indices: int32 [N * h * w], receives the proposals' head pixels b * h * w + y * w + x.  meta: int32 [N + 1 +
 *   CPN_OBJECTIVE_META_WORDS]: proposals per image, P at [N], then the number of background pixels and the CPN_OBJECTIVE_FLAG_*
 *   bits.  The caller reads meta (its one synchronisation), refuses set flags, sizes the second workspace by P.
 *  cpn_objective_proposals (asynchronous): the proposal walks, the reduction and the remaining gradients.  `present`: bit k set:
 *   term k (order above) applies.  out: float32 [9] on the device: the eight terms (NaN where not present) and the loss.
 *   g_scores / g_locations / g_fourier / g_refinement: NULL or a buffer of the map's shape; every element is written.
 *   detail_proposals [P][samples][2], detail_refined [iterations][P][samples][2] (clamped), detail_boxes [P][4]: NULL or buffers.
 *  The gradient of the refinement map is the one scatter: one contribution per (proposal, iteration, sample, bucket), sorted by
 *  element with a stable radix sort and summed in float64 in an order that depends on the sorted list alone.  No floating-point atomics: all results are
 *  bit-identical from run to run.  P * samples * iterations * (buckets > 1 ? 3 : 1) and N * buckets * H * W stay below 2^32.
 * ---------------------------------------------------------------------------------------------------------- */
#define CPN_OBJECTIVE_MAX_ITERATIONS 64
#define CPN_OBJECTIVE_META_WORDS 2
#define CPN_OBJECTIVE_FLAG_LABEL_RANGE 1 /* a pooled label above 2^24 (the reference moves labels through float32) */
#define CPN_OBJECTIVE_FLAG_LABEL_ROWS 2  /* a pooled label above K */
#define CPN_OBJECTIVE_FLAG_CLASS_RANGE 4 /* a class target outside 0 .. score_channels - 1 */
typedef struct CpnObjectiveArgs {
    const float *scores, *locations, *refinement, *fourier;
    const void *labels;
    const float *t_fourier, *t_locations, *t_contours;
    const int32_t *t_classes;
    const float *cos_table, *sin_table;
    const int32_t *bucket_index;
    const float *bucket_weight;
    const float *order_weights;
    float *g_scores, *g_locations, *g_refinement, *g_fourier;
    float *detail_proposals, *detail_refined, *detail_boxes;
    double w_fourier, w_location, w_contour, w_score_fg, w_score_bg, w_refinement, w_iou;
    int32_t N, score_channels, h, w, H, W, order_total, order, samples, K, iterations, buckets, labels_i64, reserved;
} CpnObjectiveArgs;
int64_t cpn_objective_head_workspace_bytes(int32_t N, int32_t h, int32_t w);
int cpn_objective_head(const CpnObjectiveArgs *args, int32_t *indices, int32_t *meta, void *workspace, int64_t workspace_bytes,
                       void *stream);
int64_t cpn_objective_workspace_bytes(const CpnObjectiveArgs *args, int64_t P);
int cpn_objective_proposals(const CpnObjectiveArgs *args, const int32_t *indices, int32_t P, const int32_t *meta, int32_t present,
                            void *head_workspace, void *workspace, int64_t workspace_bytes, float *out, void *stream);

/* ----------------------------------------------------------------------------------------------------------
 * Component labelling (cd.data.relabel_ / stack_labels, celldetection/data/segmentation.py:106-150, and cd.data.masks2labels,
 * celldetection/data/cpn.py:147-176; csrc/components.hip, csrc/components.h, csrc/component_rank.h).  Additions to ABI 22.
 * This text is the contract.
 *
 * The rule.  The image holds int32 elements (y, x, c) at in[(y * W + x) * pixel_stride + c * channel_stride]; a channel is
 * labelled on its own.  A pixel takes part if it is foreground.  Two neighbouring foreground pixels are linked if they are equal:
 *   CPN_COMPONENTS_EQUAL    foreground is v > 0, equal is the same value;
 *   CPN_COMPONENTS_NONZERO  foreground is v != 0, any two foreground pixels are equal.
 * Neighbours are the 4 edge neighbours (connectivity 4) or the 8 neighbours (connectivity 8).  A component is a class of the
 * transitive closure of the links.  Components are numbered first + 0, first + 1, ... by channel ascending and, within a
 * channel, by the raster index y * W + x of their first pixel (the smallest one).  Every pixel of a component receives the
 * component's number.  Pixels that take no part keep their value: zeros, and in EQUAL mode negatives.  counts = int32
 * [channels] on the device receives the number of components per channel.
 * This is skimage.measure.label(background=0) per channel (connectivity 8 = skimage's full connectivity in 2-D, which the
 * reference's relabel_ uses) with a numbering that runs on across the channels.  relabel_ skips every component that holds a
 * negative pixel; under the equal-value rule these are exactly the components of negative value: untouched and uncounted.
 * cv2.connectedComponents (masks2labels) is NONZERO mode per mask; for connectivity 8 OpenCV's default algorithm scans 2 x 2
 * blocks and may number the components of one mask in another order: the partition and the set of labels per mask are the
 * contract there, the order within a mask (raster-first, for both connectivities) is this library's own.
 *
 * Layouts: channel-interleaved (channel_stride 1, pixel_stride >= channels; the [H][W][C] label image is (C, 1)) or planar
 * (pixel_stride 1, channel_stride >= H * W; a [N][H][W] mask stack is (1, H * W)), for in and out independently; other strides
 * are CPN_E_INVALID.  out may be in (in place, same strides): then only the pixels that take part are written.
 * channels <= 65535, H * W <= 2^31 - 1, channels * ceil(H * W / 256) <= 2^31 - 2 (CPN_E_UNSUPPORTED above;
 * cpn_components_workspace_bytes returns 0 for arguments the call refuses); connectivity 4 or 8; first >= 1.
 * workspace: cpn_components_workspace_bytes(channels, H, W) bytes on the device (counters, the roots image of 4 B per pixel and
 * channel, two 8-byte words per 256 pixels, the scan's scratch).
 * More than 2^31 - 1 components, or first + components - 1 > 2^31 - 1, is CPN_E_UNSUPPORTED: nothing is written to out, no value
 * wraps.  Integer arithmetic only and no value-carrying atomics: results are bit-identical from run to run.  The call
 * synchronises the stream once (it reads the total before it numbers).  H * W = 0 zeroes counts and does nothing else.
 * ---------------------------------------------------------------------------------------------------------- */
#define CPN_COMPONENTS_EQUAL 0
#define CPN_COMPONENTS_NONZERO 1
int64_t cpn_components_workspace_bytes(int32_t channels, int32_t H, int32_t W);
int cpn_components_label(const int32_t *in, int64_t pixel_stride, int64_t channel_stride, int32_t channels, int32_t H, int32_t W,
                         int32_t connectivity, int32_t mode, int32_t first, int32_t *out, int64_t out_pixel_stride,
                         int64_t out_channel_stride, int32_t *counts, void *workspace, void *stream);

/* ---- Trainable convolution ---------------------------------------------------------------------------------
 * What celldetection_amd.nn.conv2d needs besides cpn_conv2d to train a dense stride-1 convolution (csrc/conv_train.hip,
 * csrc/wgrad_dense.h -- the one weight-gradient kernel of this section, of "Trainable grouped convolution", of "Trainable concat
 * convolution" and of "Trainable bilinear resize" --, csrc/wgrad_slabs.h).  Additions to ABI 22.  This text is the contract.
 *
 * The rule.  Supported: groups 1, stride 1, dilation 1, a square odd kernel k in {1, 3, 5, 7}, zero padding k / 2, cin and cout
 * positive multiples of 32.  Activations and weights are rounded to bf16 (round to nearest even), products accumulate in fp32,
 * the forward output and the input gradient are stored as bf16, the weight and bias gradients are fp32 sums rounded once to
 * the dtype asked for.  Activations are NHWC bf16 with the channel count as pixel stride: x [N][H][W][cin], y and dy
 * [N][H][W][cout].  dtype codes: 0 = fp32, 1 = bf16.
 *
 * Forward and input gradient are calls of cpn_conv2d (act none, one plain source, dst_stride = channels) on weights packed on the
 * device by cpn_conv_train_pack from w [cout][cin][k][k], in the layout of cpn_op_desc.weight_offset:
 *   CPN_CONV_PACK_FORWARD  [(cin / 32) * k * k items (+ one zero item when odd)][cout][32]: item (chunk, ky * k + kx), output
 *                          channel co, lane c = w[co][32 * chunk + c][ky][kx]; cin_b = cin, cout_b = cout, with the bias.
 *   CPN_CONV_PACK_DGRAD    [(cout / 32) * k * k items (+ one zero item when odd)][cin][32]: item (chunk, ky * k + kx), output
 *                          channel ci, lane c = w[32 * chunk + c][ci][k - 1 - ky][k - 1 - kx]: the taps flipped, the channel
 *                          roles swapped; cin_b = cout, cout_b = cin, no bias.  With stride 1 and padding k / 2 this conv of dy
 *                          IS the input gradient: dx[n][y][x][ci] = sum dy[n][y + ky - p][x + kx - p][co] * w[co][ci][k-1-ky][k-1-kx].
 *
 * Weight gradient: dw[co][ci][ky][kx] = sum over n, y, x of dy[n][y][x][co] * x[n][y + ky - p][x + kx - p][ci], p = k / 2, zeros
 * outside the image; bias gradient: db[co] = sum over n, y, x of dy[n][y][x][co].  The pixel range is split into slabs of
 * slab_rows consecutive image rows (of the N * H rows of the batch; the last slab may be partial, a slab may cross from one image
 * into the next; slab_rows 0 = chosen by the library).  Within a slab the pixels are reduced in ascending order, 16 per step of
 * the bf16 MFMA (v_mfma_f32_32x32x16_bf16) into one fp32 accumulator per element; the slabs' partial sums are written to the
 * workspace and added by a second kernel in ascending slab order.  No floating-point atomics: the result is bit-identical from
 * run to run.  Length of the fp32 chain of one dw element: MFMA steps per slab (= ceil(slab_rows * W / 16)) + 2 for the
 * MFMA-internal sum + one add per slab.  The bias gradient sums a slab in eight interleaved chains per channel (pixel index mod 8,
 * ascending), adds the eight in order, then the slabs in ascending order: ceil(slab_rows * W / 8) + 8 + slabs.
 * cpn_conv_wgrad_info answers without touching the device, and rejects what the launch rejects:
 *   info = {slabs, slab_rows, MFMA steps per slab, reduce chain (adds of the second kernel), chain of a bias element}.
 * dw ([cout][cin][k][k]) or db ([cout]) may be NULL: that gradient is not computed.  workspace:
 * cpn_conv_wgrad_workspace_bytes(...) bytes on the device for the same arguments (0 for arguments the call rejects).
 * N * H * W and cin * cout * k * k <= 2^31 - 1 (CPN_E_UNSUPPORTED above).
 * ---------------------------------------------------------------------------------------------------------- */
#define CPN_CONV_PACK_FORWARD 0
#define CPN_CONV_PACK_DGRAD 1
int cpn_conv_train_pack(const void *w, int32_t w_dtype, int32_t cout, int32_t cin, int32_t k, int32_t mode, void *packed,
                        void *stream);
int64_t cpn_conv_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t k, int32_t slab_rows);
int cpn_conv_wgrad(const void *x, const void *dy, int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t k,
                   int32_t slab_rows /* 0 = auto */, void *dw, int32_t dw_dtype, void *db, int32_t db_dtype, void *workspace,
                   int64_t workspace_bytes, void *stream);
int cpn_conv_wgrad_info(int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t k, int32_t slab_rows, int32_t info[5]);

/* ---- Trainable batch normalisation --------------------------------------------------------------------------
 * What celldetection_amd.nn.batch_norm runs: BatchNorm2d with an optional fused ReLU, forward and gradients
 * (csrc/batch_norm.hip, csrc/bn_slabs.h).  Additions to ABI 22.  This text is the contract.
 *
 * Layout.  x, y, dy and dx are [M][C]: M = N * H * W pixels of C channels, element (p, c) at p * C + c (a channels-last
 * [N, C, H, W] tensor), all four of one dtype, fp32 or bf16.  C is a positive multiple of 8; 1 <= M <= 2^31 - 1 (CPN_E_UNSUPPORTED
 * above); element indices are 64-bit.  dtype codes: 0 = fp32, 1 = bf16.  weight (gamma), bias (beta), the running buffers, dgamma
 * and dbeta are [C] of the dtype passed with them; weight and bias may be NULL (1 and 0).  save_mean, save_invstd, scale and
 * shift are [C] fp32.  x, y, dy, dx and the workspace are read and written 16 bytes at a time: each must start at a 16-byte
 * aligned address (CPN_E_INVALID otherwise; rows are multiples of 16 bytes because C is a multiple of 8).
 *
 * Partition.  A pixel is V = C / 8 vectors of 8 channels; the vectors are cut into channel blocks of at most 256.  A workgroup of
 * 256 lanes owns one block of vb vectors and one slab of slab_pixels consecutive pixels (the last slab may be partial;
 * slab_pixels 0 = chosen by the library, a value above M means M; a slab_pixels that gives more than 2^24 - 1 slabs, the most
 * workgroups of one launch, is CPN_E_UNSUPPORTED; the library's own choice never gives more than 2048), and moves R = floor(256 / vb) consecutive pixels per step:
 * lane l holds vector l % vb of pixel l / vb of the step, lanes >= R * vb idle.  cpn_bn_info answers without touching the device
 * and rejects what every launch rejects:
 *   info = {slabs, slab_pixels, R of the first block, channel blocks, chain of a channel sum}.
 *
 * Sums.  Every sum over pixels is an fp64 sum of terms that are exact in fp64 (x, x * x, g, g * x of fp32 or bf16 values), in a
 * fixed order: a lane adds its own pixels in ascending order, the min(R, slab pixels) lane partials of a channel are added in
 * ascending lane order, the slabs' results go to the workspace [slab][C][2] and are added in ascending slab order.  No
 * floating-point atomics: the result is bit-identical from run to run.  Chain of a channel sum: ceil(slab_pixels / R) + min(R,
 * slab_pixels) + slabs, never more than M + 1 + slabs; info reports the longest over the channel blocks + 6 for the fp64
 * operations of the finalising formulas below.
 *
 * cpn_bn_train_stats, from sum x and sum x^2, in fp64:
 *   mean = sum x / M;  var = max(sum x^2 / M - mean * mean, 0);  invstd = 1 / sqrt(var + eps);
 *   scale = gamma * invstd;  shift = beta - mean * scale,
 * save_mean = mean, save_invstd = invstd, scale and shift each rounded once to fp32.  Where a running buffer is given it is
 * updated by the same kernel, in fp64, rounded once to its dtype:
 *   running_mean = (1 - momentum) * running_mean + momentum * mean
 *   running_var  = (1 - momentum) * running_var + momentum * var * M / (M - 1)      (M = 1 with running_var: CPN_E_INVALID).
 * cpn_bn_eval_coeffs: mean = running_mean, invstd = 1 / sqrt(running_var + eps), scale and shift as above, in fp64, each rounded
 * once to fp32 into the same four vectors.
 *
 * cpn_bn_apply: t = fmaf(x, scale, shift) in fp32 with x widened exactly; y = t, or for relu != 0: t > 0 ? t : 0; a bf16 y is
 * rounded to nearest even.
 *
 * Backward: g = dy, or for relu != 0: dy where fmaf(x, scale, shift) > 0 and 0 elsewhere -- the mask is recomputed from x, scale
 * and shift by the same single fma, so it is the forward's mask bit for bit and the gradient at t == 0 is 0.  y is not read.
 * cpn_bn_backward_reduce, from sum g and sum g x, with mean = save_mean and invstd = save_invstd widened to fp64:
 *   dbeta = sum g;  dgamma = invstd * (sum g x - mean * sum g), each rounded once to its dtype (either may be NULL);
 *   coeffs (NULL or [3][C] fp32), in fp64 with the unrounded dgamma, each rounded once to fp32:
 *     a = gamma * invstd;  b = -a * invstd * dgamma / M;  c = -a * sum g / M - b * mean.
 * cpn_bn_backward_input: dx = fmaf(a, g, fmaf(b, x, c)) in fp32, rounded to the dtype of x (training: a, b, c = the three rows of
 * coeffs); with b = c = NULL dx = fmaf(a, g, 0) (eval: a = scale).
 *
 * workspace: cpn_bn_workspace_bytes(M, C, slab_pixels) bytes on the device (slabs * C * 2 fp64; 0 for arguments the call
 * rejects); a smaller one is CPN_E_WORKSPACE.  Every launch validates before it touches a pointer.
 * ---------------------------------------------------------------------------------------------------------- */
int cpn_bn_info(int64_t M, int64_t C, int64_t slab_pixels /* 0 = auto */, int64_t info[5]);
int64_t cpn_bn_workspace_bytes(int64_t M, int64_t C, int64_t slab_pixels);
int cpn_bn_train_stats(const void *x, int32_t x_dtype, int64_t M, int64_t C, int64_t slab_pixels, const void *weight,
                       int32_t weight_dtype, const void *bias, int32_t bias_dtype, void *running_mean, void *running_var,
                       int32_t running_dtype, double momentum, double eps, float *save_mean, float *save_invstd, float *scale,
                       float *shift, void *workspace, int64_t workspace_bytes, void *stream);
int cpn_bn_eval_coeffs(int64_t C, const void *weight, int32_t weight_dtype, const void *bias, int32_t bias_dtype,
                       const void *running_mean, const void *running_var, int32_t running_dtype, double eps, float *save_mean,
                       float *save_invstd, float *scale, float *shift, void *stream);
int cpn_bn_apply(const void *x, void *y, int32_t dtype, int64_t M, int64_t C, int64_t slab_pixels, const float *scale,
                 const float *shift, int32_t relu, void *stream);
int cpn_bn_backward_reduce(const void *x, const void *dy, int32_t dtype, int64_t M, int64_t C, int64_t slab_pixels,
                           const float *scale, const float *shift, int32_t relu, const float *save_mean, const float *save_invstd,
                           const void *weight, int32_t weight_dtype, void *dgamma, int32_t dgamma_dtype, void *dbeta,
                           int32_t dbeta_dtype, float *coeffs, void *workspace, int64_t workspace_bytes, void *stream);
int cpn_bn_backward_input(const void *x, const void *dy, void *dx, int32_t dtype, int64_t M, int64_t C, int64_t slab_pixels,
                          const float *scale, const float *shift, int32_t relu, const float *a, const float *b, const float *c,
                          void *stream);

/* ---- Trainable ReadOut tail ---------------------------------------------------------------------------------
 * What celldetection_amd.nn.dropout_conv1x1 runs: Dropout2d fused into a 1x1 convolution to at most 32 output channels, forward
 * and gradients (csrc/readout_tail.hip, csrc/tail_slabs.h).  Additions to ABI 22.  This text is the contract.
 *
 * Layout.  x and dx are [N][HW][cin] bf16 (a channels-last [N, cin, H, W] tensor, HW = H * W), cin a positive multiple of 32, at
 * most 1024.  weight and dw are [cout][cin], bias and db [cout], 1 <= cout <= 32, each of the dtype passed with it (0 = fp32,
 * 1 = bf16).  y and dy are [N][cout][HW] planes (a contiguous NCHW tensor), fp32 or bf16.  keep is [N][cin] bytes, non-zero = the
 * channel of that image is kept (m = 1), or NULL: everything kept.  scale is s = 1 / (1 - p), the fp32 value nearest to it (1 when
 * nothing is dropped, 0 for p = 1); it must be finite and not negative.  N * HW <= 2^31 - 1 (CPN_E_UNSUPPORTED above).  x, dx and
 * the workspace are read and written 16 bytes at a time: each must start at a 16-byte aligned address; y and dy at a multiple of
 * their element size (CPN_E_INVALID otherwise).
 *
 * Forward.  acc[n][q][o] = sum over c of m[n][c] * bf16(W[o][c]) * x[n][q][c], an fp32 sum on the bf16 MFMA
 * (v_mfma_f32_32x32x16_bf16, 16 channels per step in ascending order): the weight operand is masked per image, so a dropped
 * channel contributes an exact zero and x * s is never rounded.  y = fmaf(acc, s, bias) is rounded once to the dtype of y (bias
 * widened exactly, 0 without one).  Chain of acc: cin / 16 + 2 (the MFMA-internal sum).  The pixels of an image are cut into tiles
 * of 32; a tile never holds pixels of two images.
 *
 * Backward.  Every use of dy reads its bf16 rounding (round to nearest even), converted inside the kernel from the fp32 or bf16
 * planes.
 *   dx[n][q][c] = m[n][c] * s * sum over o of bf16(W[o][c]) * bf16(dy[n][o][q]): an fp32 sum on the MFMA (K = cout padded to 16 or
 *   32: one or two steps), one multiply by s, rounded once to bf16; exactly 0 for a dropped channel.
 *   dw[o][c] = s * sum over n of m[n][c] * sum over q of bf16(dy[n][o][q]) * x[n][q][c];  db[o] = sum of bf16(dy[n][o][q]).
 * Pixels are reduced on the MFMA in slabs that never cross an image: image n is cut into ceil(HW / slab_pixels) slabs of
 * slab_pixels consecutive pixels (the last may be partial; slab_pixels 0 = chosen by the library, a value above HW means HW; more
 * than 2^24 - 1 slabs is CPN_E_UNSUPPORTED).  Within a slab the pixels are reduced in ascending order, 16 per MFMA step, into one
 * fp32 accumulator per element; a slab's fp32 partial goes to the workspace, and a second kernel adds the slabs in ascending
 * (n, slab) order, skipping the slabs of the images whose channel was dropped (a multiplication by 0 or 1, exact), multiplies by
 * s once and rounds once to the dtype of dw.  Chain of a dw element: MFMA steps per slab (= ceil(slab_pixels / 16)) + 2 for the
 * MFMA-internal sum + the reduce chain (one add per slab + the multiplication by s).  The bias gradient sums a slab in eight
 * interleaved chains per channel (pixel index inside the slab mod 8, ascending), adds the eight in order, then the slabs in
 * ascending order: ceil(slab_pixels / 8) + 8 + slabs; it is neither masked nor scaled.  No floating-point atomics: the result is
 * bit-identical from run to run.  Rows cout ... 31 of the MFMA tile read zeros and are never written: nothing behind weight, bias,
 * dy, y, dw or db is touched.
 *
 * cpn_tail_info answers without touching the device and rejects what the launches reject:
 *   info = {slabs, slab_pixels, MFMA steps per slab, reduce chain, chain of a bias element, forward chain, slabs per image,
 *           MFMA steps of a dx element}.
 * cpn_tail_backward: dx, dw and db may each be NULL: that gradient is not computed, and what only it reads is not read (x for dw,
 * weight for dx).  workspace: cpn_tail_workspace_bytes(...) bytes on the device for the same arguments (slabs * (cin * cout +
 * cout) fp32; 0 for arguments the call rejects), needed for dw or db; a smaller one is CPN_E_WORKSPACE.  Every launch validates
 * before it touches a pointer.
 * ---------------------------------------------------------------------------------------------------------- */
int cpn_tail_info(int64_t N, int64_t HW, int32_t cin, int32_t cout, int64_t slab_pixels /* 0 = auto */, int64_t info[8]);
int64_t cpn_tail_workspace_bytes(int64_t N, int64_t HW, int32_t cin, int32_t cout, int64_t slab_pixels);
int cpn_tail_forward(const void *x, const void *weight, int32_t weight_dtype, const void *bias, int32_t bias_dtype,
                     const uint8_t *keep, float scale, int64_t N, int64_t HW, int32_t cin, int32_t cout, void *y, int32_t y_dtype,
                     void *stream);
int cpn_tail_backward(const void *x, const void *dy, int32_t dy_dtype, const void *weight, int32_t weight_dtype, const uint8_t *keep,
                      float scale, int64_t N, int64_t HW, int32_t cin, int32_t cout, int64_t slab_pixels, void *dx, void *dw,
                      int32_t dw_dtype, void *db, int32_t db_dtype, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- Trainable grouped convolution --------------------------------------------------------------------------
 * What celldetection_amd.nn.grouped_conv2d needs besides cpn_conv2d to train the 3x3 conv2 of a ResNeXt bottleneck block
 * (csrc/grouped_conv_train.hip, csrc/grouped_conv.h, csrc/wgrad_slabs.h, csrc/wgrad_bias.h; the weight gradient's slab kernel is
 * the dense one's, csrc/wgrad_dense.h with csrc/mfma_frag.h).  Additions to ABI 22.  This text is the contract.
 *
 * The rule.  A conv of C -> C channels in groups of cig = C / groups channels, cig in {4, 8, 16, 32, 64}, kernel 3x3, zero padding
 * 1, dilation 1, stride 1 or 2.  It runs as bundles = C / bw block-diagonal dense convs of bw -> bw channels: bw = 32 for
 * cig <= 32 (32 / cig groups per bundle), bw = 64 for cig = 64 (one group per bundle); C is a positive multiple of bw.  Arithmetic
 * and layout are those of the "Trainable convolution" section: bf16 operands (round to nearest even), fp32 accumulation, NHWC bf16
 * activations with C as pixel stride (x and dx [N][Hin][Win][C]; y and dy [N][Hout][Wout][C], Hout = (Hin - 1) / stride + 1),
 * dw [C][cig][3][3] and db [C] fp32 sums rounded once to the dtype asked for.  dtype codes: 0 = fp32, 1 = bf16.
 *
 * Forward and input gradient are calls of cpn_conv2d (bundles, cin_b = cout_b = bw, c0_used = C, kh = kw = 3, pad 1, act none,
 * one plain source, dst_stride = C) on weights packed on the device by cpn_grouped_conv_pack from w [C][cig][3][3], in the layout
 * of cpn_op_desc.weight_offset: [bundle][item = (32-channel chunk of the bundle, tap ky * 3 + kx)][bw][32], (bw / 32) * 9 items
 * and one zero item behind an odd count IN EVERY BUNDLE (bw = 32: 9 + 1).  With oc the record's output channel and rc = 32 chunk +
 * lane its reduced channel, both inside the bundle:
 *   CPN_CONV_PACK_FORWARD  w[bw bundle + oc][rc mod cig][ky][kx] where oc / cig == rc / cig, an exact zero elsewhere; stride 1 or
 *                          2 in the descriptor, with the bias.
 *   CPN_CONV_PACK_DGRAD    w[bw bundle + rc][oc mod cig][2 - ky][2 - kx] where oc / cig == rc / cig, an exact zero elsewhere: the
 *                          taps flipped, the channel roles swapped inside each group; stride 1, no bias.  At stride 1 this conv of
 *                          dy IS the input gradient.
 *
 * Stride 2, by zero-dilation.  cpn_grouped_conv_dilate writes dz [N][Hin][Win][C] with dz[n][2 i][2 j] = dy[n][i][j] and exact
 * zeros elsewhere (every 16-byte unit of dz written once; 2 (Hout - 1) <= Hin - 1 for even and odd Hin).  The stride-2 output is
 * y[i][j] = sum w[ky][kx] x[2 i + ky - 1][2 j + kx - 1], so
 *   dx[u][v] = sum over (i, j, ky, kx) with 2 i + ky - 1 = u, 2 j + kx - 1 = v of dy[i][j] w[ky][kx]
 *            = sum over ky, kx of dz[u - ky + 1][v - kx + 1] w[ky][kx]: the stride-1 dgrad conv of dz;
 *   dw[ky][kx] = sum over i, j of dy[i][j] x[2 i + ky - 1][2 j + kx - 1] = sum over all (u, v) of dz[u][v] x[u + ky - 1][v + kx - 1]:
 *            the stride-1 weight gradient of (x, dz), the odd positions contributing exact zeros.
 * The bias gradient sums dy itself.  Known limit: 4 x the minimal work and one more tensor of x's size.
 *
 * Weight gradient: dw[co][cl][ky][kx] = sum over n, y, x of dz[n][y][x][co] * x[n][y + ky - 1][x + kx - 1][cig (co / cig) + cl]
 * (stride 1: dz = dy), zeros outside the image.  Only the diagonal 32 x 32 fragments of the (co, ci) matrix are computed: a wave
 * owns one of them (bw = 32: one bundle; bw = 64: one of the four of a group), a workgroup four of them for one filter row ky.
 * The pixel range is split into slabs of slab_rows consecutive image rows (of the N * Hin rows; the last slab may
 * be partial, a slab may cross from one image into the next; slab_rows 0 = chosen by the library).  Within a slab the pixels are
 * reduced in ascending order, 16 per step of v_mfma_f32_32x32x16_bf16, into one fp32 accumulator per element; the slabs' partial
 * sums go to the workspace and a second kernel adds them in ascending slab order, reads only the entries whose input and output
 * channel share a group (the off-group products of a 32-wide bundle never reach dw) and rounds once.  No floating-point atomics:
 * the result is bit-identical from run to run.  Chain of a dw element: MFMA steps per slab (= ceil(slab_rows * Win / 16)) + 2 for
 * the MFMA-internal sum + one add per slab.  The bias gradient is that of the "Trainable convolution" section on dy, partitioned
 * by the same slab_rows over its N * Hout rows: ceil(slab_rows * Wout / 8) + 8 + slabs.
 * cpn_grouped_conv_wgrad_info answers without touching the device, and rejects what the launch rejects:
 *   info = {slabs, slab_rows, MFMA steps per slab, reduce chain (adds of the second kernel), chain of a bias element}.
 * cpn_grouped_conv_wgrad: dz is the gradient at the input's size (dy itself at stride 1, the dilated one at stride 2), read for
 * dw together with x; dy is read for db only.  dw or db may be NULL: that gradient is not computed and its operands may be NULL.
 * x and dz start at 16-byte aligned addresses (CPN_E_INVALID otherwise).  workspace: cpn_grouped_conv_wgrad_workspace_bytes(...)
 * bytes on the device for the same arguments (0 for arguments the call rejects); a smaller one is CPN_E_WORKSPACE.
 * N * Hin * Win <= 2^31 - 1 and N * Hin * Win * C < 2^30 (CPN_E_UNSUPPORTED above: the limit of cpn_conv2d's sources).  Every
 * launch validates before it touches a pointer.
 * ---------------------------------------------------------------------------------------------------------- */
int cpn_grouped_conv_pack(const void *w, int32_t w_dtype, int32_t C, int32_t cig, int32_t mode /* CPN_CONV_PACK_* */, void *packed,
                          void *stream);
int cpn_grouped_conv_dilate(const void *dy, int32_t N, int32_t Hin, int32_t Win, int32_t C, void *dz, void *stream);
int64_t cpn_grouped_conv_wgrad_workspace_bytes(int32_t N, int32_t Hin, int32_t Win, int32_t C, int32_t cig, int32_t stride,
                                               int32_t slab_rows);
int cpn_grouped_conv_wgrad_info(int32_t N, int32_t Hin, int32_t Win, int32_t C, int32_t cig, int32_t stride, int32_t slab_rows,
                                int32_t info[5]);
int cpn_grouped_conv_wgrad(const void *x, const void *dz, const void *dy, int32_t N, int32_t Hin, int32_t Win, int32_t C, int32_t cig,
                           int32_t stride, int32_t slab_rows /* 0 = auto */, void *dw, int32_t dw_dtype, void *db, int32_t db_dtype,
                           void *workspace, int64_t workspace_bytes, void *stream);

/* ---- Trainable bottleneck block -----------------------------------------------------------------------------
 * What celldetection_amd.nn.Bottleneck needs besides the four sections above to run a ResNeXt bottleneck block, residual add and
 * strided shortcut included (csrc/batch_norm.hip, csrc/grouped_conv_train.hip, csrc/grouped_conv.h).  Additions to ABI 22.  This
 * text is the contract.
 *
 * A. Norm + residual add (+ ReLU): y = relu(bn(x) + r).  Layout, partition, dtype codes, alignment and limits are those of the
 * "Trainable batch normalisation" section; r, y and g are [M][C] of x's dtype.
 *   cpn_residual_bn_apply: t = fmaf(x, scale, shift) in fp32 with x widened exactly; s = t + r, an fp32 add with r widened exactly
 *   (a rounding of its own: two roundings in fp32); y = s, or for relu != 0: s > 0 ? s : 0; a bf16 y is rounded once to nearest
 *   even.  Three passes over the tensor: read x, read r, write y.
 *   Backward.  The mask comes from the stored output: g = dy where y > 0 (in the stored dtype) and 0 elsewhere; r is not needed.
 *   cpn_residual_bn_backward_reduce, relu != 0: reads x, dy and y, writes g once -- g IS the residual's gradient, bit for bit --
 *   and accumulates sum g and sum g x in fp64 in the order and the workspace layout of cpn_bn_backward_reduce; the same finalising
 *   kernel gives dgamma, dbeta and coeffs (all three NULL: g alone is written).  scale and shift are not read.  relu == 0: g = dy,
 *   y and g are not looked at and nothing is written to g: the call is cpn_bn_backward_reduce with relu = 0.
 *   cpn_bn_backward_input with relu = 0 on g then gives dx.  Passes backward: 4 + 3 = 7.
 *
 * B. Strided 1x1 shortcut conv, stride 2, no padding.  The forward is cpn_conv2d with kh = kw = 1, pad 0, stride 2 on x itself
 * (the pointwise kernel gathers only its outputs): y [N][Hout][Wout][cout], Hout = (Hin - 1) / 2 + 1.  Input gradient: the
 * stride-1 1x1 dgrad conv of dy at the output's size, then cpn_grouped_conv_dilate to the input's size (the even grid, exact zeros
 * elsewhere).  Weight gradient: dw[o][c] = sum dy[i][j][o] x[2 i][2 j][c] = cpn_conv_wgrad(xs, dy, k = 1) with
 *   cpn_subsample2d: xs [N][Hout][Wout][C], xs[n][i][j] = x[n][stride i][stride j], bf16 NHWC, 16 bytes per lane, every unit of xs
 *   written once, for even and odd Hin / Win.  C a positive multiple of 8, stride 2, N, Hin, Win >= 1 (CPN_E_INVALID otherwise);
 *   N * Hin * Win <= 2^31 - 1 and N * Hin * Win * C < 2^30 (CPN_E_UNSUPPORTED above); x and xs start at 16-byte aligned addresses
 *   (CPN_E_INVALID).  It validates before it touches a pointer.
 *
 * C. Block-input gradient: the sum of the gradients of conv1's input and of the skip is the residual operand of the dgrad conv --
 * cpn_conv2d with res = dskip, res_stride = cin: dx = round_bf16(fp32 conv sum + dskip), one rounding.  No entry point of its own.
 * ---------------------------------------------------------------------------------------------------------- */
int cpn_residual_bn_apply(const void *x, const void *r, void *y, int32_t dtype, int64_t M, int64_t C, int64_t slab_pixels,
                          const float *scale, const float *shift, int32_t relu, void *stream);
int cpn_residual_bn_backward_reduce(const void *x, const void *dy, const void *y, void *g, int32_t dtype, int64_t M, int64_t C,
                                    int64_t slab_pixels, const float *scale, const float *shift, int32_t relu,
                                    const float *save_mean, const float *save_invstd, const void *weight, int32_t weight_dtype,
                                    void *dgamma, int32_t dgamma_dtype, void *dbeta, int32_t dbeta_dtype, float *coeffs,
                                    void *workspace, int64_t workspace_bytes, void *stream);
int cpn_subsample2d(const void *x, int32_t N, int32_t Hin, int32_t Win, int32_t C, int32_t stride, void *xs, void *stream);

/* ---- Trainable concat convolution ---------------------------------------------------------------------------
 * What celldetection_amd.nn.cat_conv2d needs besides cpn_conv2d and the "Trainable convolution" section to train the first conv
 * of a U-Net decoder level (csrc/cat_conv_train.hip, csrc/nearest_adjoint.h, csrc/wgrad_dense.h, csrc/wgrad_slabs.h,
 * csrc/wgrad_bias.h).  Additions to ABI 22.  This text is the contract.
 *
 * The function.  y = conv(cat(x0, R(x1)), w) + b with x0 [N][H][W][C0] (the lateral) first and x1 [N][h][w][C1] (the top) second,
 * 1 <= h <= H, 1 <= w <= W, bf16 NHWC; w [cout][C0 + C1][k][k], k square and odd, stride 1, padding k / 2 with zeros; C0, C1 and
 * cout positive multiples of 32.  R is PyTorch's 'nearest' resize to H x W: R(x1)[n][y][x] = x1[n][src_y(y)][src_x(x)] with
 * src(d) = min((int) floorf((float) d * scale), in - 1), scale = (float) in / (float) out -- nearest_src of csrc/cpn_kernels.h,
 * restated as na_src in csrc/nearest_adjoint.h.  Equal sizes make R the identity.  The bridge level has no lateral: C0 = 0,
 * x0 = NULL, and H = 2 h, W = 2 w exactly.
 *
 * Arithmetic.  Operands are rounded to bf16 (round to nearest even), sums are fp32, every stored value is rounded once.
 *
 * Forward.  cpn_conv2d_sized with src1 = x1, up1 = 1, c0_used = C0, cin_b = C0 + C1 on the forward pack of w (cpn_conv_train_pack):
 * the loader resizes the second source; neither R(x1) nor the concatenated tensor is ever written.
 *   cpn_conv2d_sized: cpn_conv2d plus stored[6] = {Hs0, Ws0, Hs1, Ws1, Hr, Wr}, the sizes at which the two sources and the residual
 *   are stored (looked at for a source with up != 0 and a residual with res_up != 0 only; cpn_conv2d assumes Hin >> 1 x Win >> 1).
 *   A resized source of less than 1 or more than Hin x Win pixels, or stored == NULL: CPN_E_INVALID before a pointer is read.
 * The bridge level is cpn_conv2d with the lone source resized (up0 = 1: exactly x2).
 *
 * Input gradients.  dcat = the stride-1 conv of dY with the taps flipped and the channel roles swapped, as in the "Trainable
 * convolution" section, run as two convs on the dgrad packs of w[:, :C0] and w[:, C0:]:
 *   d_x0 = dcat[:, :C0], written directly, one rounding;
 *   T = dcat[:, C0:], bf16 at the lateral's size [N][H][W][C1];
 *   d_x1[n][i][j][c] = the sum of T[n][y][x][c] over all (y, x) with src_y(y) = i and src_x(x) = j (the footprint of (i, j)), the
 *   adds in fp32 in ascending row-major (y, x) order, rounded once to bf16; an empty footprint gives an exact zero.  src is the
 *   function of the forward, so forward and backward are exact adjoints at every size.  src is non-decreasing: a footprint is the
 *   product of two contiguous ranges, [na_first(i), na_first(i + 1)) per axis.
 *   cpn_nearest_sum: d_x1 from T.  16 bytes (8 channels) per lane; C a positive multiple of 8, N, H, W >= 1, 1 <= h <= H,
 *   1 <= w <= W (CPN_E_INVALID otherwise), N * H * W <= 2^31 - 1 (CPN_E_UNSUPPORTED above), t and dst 16-byte aligned.
 * A conv whose gradient is not asked for is not run.
 *
 * Weight and bias gradients.  dw[co][ci][ky][kx] = sum over pixels p of dY[p][co] * X[p + (ky - pad) * W + (kx - pad)][ci] with
 * zeros outside the image, where X is the VIRTUAL concat: channels ci < C0 come from x0 at the pixel, channels ci >= C0 from x1 at
 * the pixel's source pixel.  Partition, chains and rounding are those of cpn_conv_wgrad: slabs of slab_rows image rows of the
 * N * H rows, 16 pixels per MFMA step in one fp32 accumulator per output, then the slabs' partial sums added in ascending slab
 * order (+ one add per slab), rounded once to dw_dtype; db likewise from dY alone.  No floating-point atomics: bit-identical from
 * run to run.  A 32-channel block of the 64-channel tile belongs to one source; the source pixel of each staged row is computed
 * once per 128-pixel chunk into an LDS table; R(x1) is never materialised.
 *   cpn_cat_conv_wgrad_info / cpn_cat_conv_wgrad_workspace_bytes / cpn_cat_conv_wgrad: the argument order of cpn_conv_wgrad_info /
 *   _workspace_bytes / cpn_conv_wgrad with (x0, x1) in place of x and (c0, c1, h1, w1) in place of cin.  info[5] = {slabs,
 *   slab_rows, MFMA steps of the largest slab, reduce chain, bias chain}; the chain of one dw element is info[2] + 2 + info[3].
 *   c0 = 0 with x0 = NULL is the bridge level.  CPN_E_INVALID: N, H, W < 1, h1 / w1 outside 1 ... H / 1 ... W, c0 not 0 or a
 *   positive multiple of 32, c1 or cout not positive multiples of 32, k not in {1, 3, 5, 7}, slab_rows < 0, x0 null with c0 > 0 or
 *   the reverse, a null or unaligned pointer, an unknown dtype code.  CPN_E_UNSUPPORTED: more than 2^31 - 1 pixels or weights, more
 *   than 65535 tiles of 64 x 64 channels, a chain longer than 2^31 - 1.  CPN_E_WORKSPACE: a workspace smaller than
 *   cpn_cat_conv_wgrad_workspace_bytes = slabs * ((c0 + c1) * cout * k * k + cout) * 4.  Every call validates before it reads a
 *   pointer.
 *
 * Saved for backward by cat_conv2d: x0 and x1 (bf16, x1 at its own low resolution) and w.  Known limits: T is written and read
 * once (no footprint sum in the dgrad epilogue, no 4 x 4 stride-2 adjoint for the exact x2); the forward is not decomposed into
 * sub-pixel phases; cpn_nearest_sum walks a footprint serially in one lane, so a tiny top under a large lateral (h = w = 1 at the
 * extreme) leaves a handful of lanes reading the whole image: correct at any ratio, fast at the small ratios of a decoder.
 * ---------------------------------------------------------------------------------------------------------- */
int cpn_conv2d_sized(const cpn_op_desc *op, const void *src0, int32_t c0_stride, const void *src1, int32_t c1_stride,
                     const void *res, int32_t res_stride, void *dst, int32_t dst_stride, int32_t N, int32_t Hin, int32_t Win,
                     const int32_t stored[6], const void *weights, const float *bias, void *stream);
int64_t cpn_cat_conv_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t c0, int32_t c1, int32_t h1, int32_t w1,
                                           int32_t cout, int32_t k, int32_t slab_rows);
int cpn_cat_conv_wgrad_info(int32_t N, int32_t H, int32_t W, int32_t c0, int32_t c1, int32_t h1, int32_t w1, int32_t cout, int32_t k,
                            int32_t slab_rows, int32_t info[5]);
int cpn_cat_conv_wgrad(const void *x0, const void *x1, const void *dy, int32_t N, int32_t H, int32_t W, int32_t c0, int32_t c1,
                       int32_t h1, int32_t w1, int32_t cout, int32_t k, int32_t slab_rows /* 0 = auto */, void *dw, int32_t dw_dtype,
                       void *db, int32_t db_dtype, void *workspace, int64_t workspace_bytes, void *stream);
int cpn_nearest_sum(const void *t, int32_t N, int32_t H, int32_t W, int32_t C, void *dst, int32_t h, int32_t w, void *stream);

/* ---- Trainable stem and max-pool ----------------------------------------------------------------------------
 * What celldetection_amd.nn.stem_conv2d and nn.max_pool2d run: the first two modules of a ResNet / ResNeXt encoder,
 * Conv2d(C <= 4 -> 32 | 64, 7x7, stride 2, padding 3) and MaxPool2d(3, 2, 1), and the MaxPool2d(2, 2) of the U-Net encoders
 * (csrc/stem_train.hip, csrc/image_train.h, csrc/stem_mfma.h -- the forward loop, shared with csrc/stem.hip --, csrc/mfma_frag.h,
 * csrc/pool_train.hip, csrc/pool_adjoint.h, csrc/wgrad_slabs.h, csrc/wgrad_bias.h).  Additions to ABI 22.  This text is the contract.
 *
 * The stem's input is the padded 4-channel tensor Xp, bf16 [N][H + 6][W + 8][4] with a zero border (3 rows / columns in front) and
 * zeros in the channels c >= C, as cpn_convert_input_stem writes it (range_flag = NULL: a training input need not lie in [0, 1]).
 * Hout = (H - 1) / 2 + 1, Wout = (W - 1) / 2 + 1.  The 32 values (kx 0..7, c 0..3) that output pixel (oy, ox) meets in filter row
 * ky are the 64 contiguous bytes at Xp[n][2 oy + ky][2 ox]; every such read lies inside Xp, the last row of the last image
 * included.  Arithmetic: operands are rounded to bf16 (round to nearest even), sums are fp32, every stored value is rounded once.
 *
 *   cpn_stem_train_pack: weight [cout][cin][7][7] (weight_dtype 0 = fp32 | 1 = bf16) -> packed [7][cout][32] bf16: filter row,
 *   output channel, (kx 0..7, c 0..3), zeros at kx = 7 and c >= cin -- the layout of CPN_OP_STEM7.  Round to nearest even, fp32
 *   subnormals included; bf16 weights are copied.  Runs on the device every step.  cout 32 | 64, 1 <= cin <= 4 (CPN_E_INVALID).
 *
 *   cpn_stem_train_forward: y[n][oy][ox][co] = sum over (ky, kx, c) of Xp[n][2 oy + ky][2 ox + kx][c] * packed[ky][co][kx][c]
 *   (+ bias[co], fp32, may be NULL), bf16 NHWC [N][Hout][Wout][cout], no activation.  The loop of the inference stem
 *   (csrc/stem_mfma.h): 14 v_mfma_f32_32x32x16_bf16 steps per output in one fp32 accumulator, + 2 for the MFMA-internal sum, + the
 *   bias add, one rounding to bf16.
 *
 *   cpn_stem_wgrad: dw[co][c][ky][kx] = sum over (n, oy, ox) of dY[n][oy][ox][co] * Xp[n][2 oy + ky][2 ox + kx][c] for kx < 7 and
 *   c < cin; dY bf16 NHWC [N][Hout][Wout][cout].  The reduction index is the flat output pixel p = (n Hout + oy) Wout + ox.  Slabs
 *   of slab_rows output rows of the N * Hout rows (0 = auto: at most 256 slabs of equal size; csrc/wgrad_slabs.h); inside a slab
 *   the pixels in ascending order, 16 per MFMA step, in ONE fp32 accumulator per element (no cross-wave sum: one wave owns a filter
 *   row of a slab from its first pixel to its last); pixels behind a slab's end are zeros in both operands.  The slabs' partial
 *   sums, workspace [slab][7][cout][32] fp32, are added in ascending slab order (+ one add per slab) and rounded once to dw_dtype;
 *   the columns kx = 7 and c >= cin are never read, so they never reach dw.  db[co] = the sum of dY, by the bias kernels of
 *   cpn_conv_wgrad: 8 interleaved chains per slab added in order, then the slabs in ascending slab order.  No floating-point
 *   atomics: bit-identical from run to run.  There is no input gradient.
 *   cpn_stem_wgrad_info: info[5] = {slabs, slab_rows, MFMA steps of the largest slab, reduce chain, bias chain}; the chain of one
 *   dw element is info[2] + 2 + info[3].  cpn_stem_wgrad_workspace_bytes = slabs * (7 * cout * 32 + cout) * 4.  Both answer
 *   without a GPU.  H and W are the IMAGE's size.
 *   CPN_E_INVALID: N, H, W < 1, cout not 32 | 64, cin outside 1 ... 4, slab_rows < 0, a null or unaligned (16 bytes) pointer, dw
 *   and db both null, an unknown dtype code.  CPN_E_UNSUPPORTED: more than 2^31 - 1 pixels in Xp.  CPN_E_WORKSPACE: a workspace
 *   smaller than cpn_stem_wgrad_workspace_bytes.  Every call validates before it reads a pointer.
 *
 * The pool.  (k, stride, pad) = (3, 2, 1) or (2, 2, 0); x [N][H][W][C] NHWC, dtype 0 = fp32 | 1 = bf16, C a positive multiple of
 * 8, 16 bytes per lane; Hout = (H + 2 pad - k) / stride + 1 >= 1, Wout likewise.  Inputs are finite: NaN is outside the contract.
 *
 *   cpn_maxpool2d_indexed: y [N][Hout][Wout][C] in x's dtype and index, one uint8 per element of y.  Tie rule (torch's): the
 *   window's positions (oy stride - pad + ty, ox stride - pad + tx) are scanned in raster order of (ty, tx); positions outside the
 *   image do not exist (the window is cut at the border, not clamped); a position takes the window over only when its value is
 *   strictly greater, so the first maximum wins (-0 and +0 are equal: the first of them).  index = ty * k + tx of the winner.  y is
 *   the winner's value, bit for bit what cpn_maxpool2d gives.
 *
 *   cpn_maxpool2d_backward: dx [N][H][W][C] from dY and index.  A lane owns 16 bytes of one input pixel (iy, ix) and visits the at
 *   most 2 x 2 windows that cover it, in raster order of (oy, ox); where index[oy][ox] names the tap this pixel is in that window it
 *   adds dY[oy][ox] in fp32 (at most 4 terms: 3 adds), and rounds once to the tensor's dtype.  A pixel no window names, or no
 *   window covers (the odd last row or column at (2, 2, 0)), gets an exact 0.  No atomics, no scatter: bit-identical from run to
 *   run.  Which windows cover a pixel and which tap it is there: csrc/pool_adjoint.h (integer only, also compiled for the host).
 *   CPN_E_INVALID: N, H, W < 1, C not a positive multiple of 8, an unknown dtype code, another geometry, an axis shorter than a
 *   window, a null or unaligned (16 bytes) pointer.  CPN_E_UNSUPPORTED: more than 2^31 - 1 pixels or workgroups.
 *
 * Saved for backward: by stem_conv2d Xp alone (4 channels for the image's 3: a third more than the image in bf16, plus the border), by
 * max_pool2d the uint8 index alone.  Known limits: no input gradient of the stem; batch-norm statistics are not folded into the
 * stem's epilogue; the pool is not fused into the norm's apply; the weight gradient stages every pixel's 64 bytes of Xp on their
 * own (the overlap of neighbouring pixels is left to the caches); 7x7 / stride 2 only (the 3x3 stride-1 first conv of the U-Net
 * encoders is the "Trainable image conv" section below).
 * ---------------------------------------------------------------------------------------------------------- */
int cpn_stem_train_pack(const void *weight, int32_t weight_dtype, int32_t cout, int32_t cin, void *packed, void *stream);
int cpn_stem_train_forward(const void *xp, const void *packed, const float *bias, int32_t N, int32_t H, int32_t W, int32_t cout,
                           void *y, void *stream);
int cpn_stem_wgrad_info(int32_t N, int32_t H, int32_t W, int32_t cout, int32_t slab_rows, int32_t info[5]);
int64_t cpn_stem_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t cout, int32_t slab_rows);
int cpn_stem_wgrad(const void *xp, const void *dy, int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout,
                   int32_t slab_rows /* 0 = auto */, void *dw, int32_t dw_dtype, void *db, int32_t db_dtype, void *workspace,
                   int64_t workspace_bytes, void *stream);
int cpn_maxpool2d_indexed(const void *x, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t stride,
                          int32_t pad, void *y, void *index, void *stream);
int cpn_maxpool2d_backward(const void *dy, const void *index, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k,
                           int32_t stride, int32_t pad, void *dx, void *stream);

/* ---- Trainable image conv -----------------------------------------------------------------------------------
 * What celldetection_amd.nn.image_conv2d runs: the first module of the reference's UNetEncoder (models/unet.py:29-58; CpnU22,
 * CpnSlimU22, CpnWideU22, U17, U12), Conv2d(C <= 4 -> 32 | 64 | 128, 3x3, stride 1, padding 1) on the image itself
 * (csrc/image_conv_train.hip, csrc/image_train.h, csrc/mfma_frag.h, csrc/stem_mfma.h -- its epilogue only --, csrc/wgrad_slabs.h,
 * csrc/wgrad_bias.h).  Additions to ABI 22.  This text is the contract.
 *
 * The conv's input is the padded 4-channel tensor Xq, bf16 [N][H + 2][Wq = W + 3][4] with a zero border (one row and one column
 * in front, one row and two columns behind) and zeros in the channels c >= C.  The output has the image's size H x W.  The 16
 * values (kx 0..3, c 0..3) that output pixel (y, x) meets in filter row ky are the 32 contiguous bytes at Xq[n][y + ky][x]; every
 * such read lies inside Xq, the last row of the last image included (it ends at Xq's last byte).  Arithmetic: operands are rounded
 * to bf16 (round to nearest even), sums are fp32, every stored value is rounded once.  Image values must be finite: the column
 * kx = 3 multiplies a real neighbouring pixel (x + 2 of the image, where it exists) by a zero weight, as the stem's kx = 7 does,
 * and an infinity or a NaN there would reach the sum.
 *
 *   cpn_image_conv_pad: src fp32 NCHW [N][C][H][W] -> Xq.  Round to nearest even, fp32 subnormals included (NaN stays NaN); what
 *   cpn_convert_input_stem with range_flag = NULL does for the stem's border.  1 <= C <= 4.
 *
 *   cpn_image_conv_pack: weight [cout][cin][3][3] (weight_dtype 0 = fp32 | 1 = bf16) -> packed [3][cout][16] bf16: filter row,
 *   output channel, (kx 0..3, c 0..3), zeros at kx = 3 and c >= cin.  Round to nearest even, fp32 subnormals included; bf16 weights
 *   are copied.  Runs on the device every step.  cout 32 | 64 | 128, 1 <= cin <= 4 (CPN_E_INVALID).
 *
 *   cpn_image_conv_forward: y[n][y][x][co] = sum over (ky, kx, c) of Xq[n][y + ky][x + kx][c] * packed[ky][co][kx][c] (+ bias[co],
 *   fp32, may be NULL), bf16 NHWC [N][H][W][cout], no activation.  A wave owns a fragment of 32 consecutive pixels of one image row
 *   at a time (persistent waves, grid-stride over the N * H * ceil(W / 32) fragments, at most 4 | 3 | 2 workgroups of four waves
 *   per CU for cout 32 | 64 | 128) and every output channel of it: one v_mfma_f32_32x32x16_bf16 step per filter row, so 3 steps per output in one fp32 accumulator, + 2
 *   for the MFMA-internal sum, + the bias add, one rounding to bf16.  Both operands come straight from global memory (the weights
 *   once per wave, the next fragment's pixels before this fragment's products); a lane stores 16 bytes = 8 consecutive channels of
 *   its pixel.  Lanes behind a row's end recompute its last pixel and store nothing.
 *
 *   cpn_image_conv_wgrad: dw[co][c][ky][kx] = sum over (n, y, x) of dY[n][y][x][co] * Xq[n][y + ky][x + kx][c] for kx < 3 and
 *   c < cin; dY bf16 NHWC [N][H][W][cout].  The reduction index is the flat output pixel p = (n H + y) W + x.  Slabs of slab_rows
 *   image rows of the N * H rows (0 = auto: at most 512 slabs of equal size; csrc/wgrad_slabs.h); inside a slab the pixels in
 *   ascending order, 16 per MFMA step, in ONE fp32 accumulator per element (no cross-wave sum).  A workgroup of four waves owns a
 *   slab and all three filter rows.  Per chunk of 128 pixels it stages the dY rows in LDS once for all three filter rows, next to
 *   two images of the pixels' Xq values: image 0 holds the 32 bytes of filter rows 0 and 1 side by side, image 1 those of filter row
 *   2 and zeros.  Wave w owns image w % 2 and the 32-channel blocks w / 2 and w / 2 + 2 of dY, from the slab's first pixel to its
 *   last (with cout = 32 waves 2 and 3 stage only); the next chunk's global loads are issued before this chunk's products.  Pixels
 *   behind a slab's end are zeros in both operands.  The slabs' partial sums, workspace [slab][3][cout][16] fp32, are added in
 *   ascending slab order (+ one add per slab) and rounded once to dw_dtype; the columns kx = 3 and c >= cin are never read, so they
 *   never reach dw.  db[co] = the sum of dY, by the bias kernels of cpn_conv_wgrad: 8 interleaved chains per slab added in order,
 *   then the slabs in ascending slab order.  No floating-point atomics: bit-identical from run to run.  There is no input gradient.
 *   cpn_image_conv_wgrad_info: info[5] = {slabs, slab_rows, MFMA steps of the largest slab, reduce chain, bias chain}, what it means
 *   for the stem; the chain of one dw element is info[2] + 2 + info[3].  cpn_image_conv_wgrad_workspace_bytes = slabs *
 *   (3 * cout * 16 + cout) * 4.  Both answer without a GPU.
 *   CPN_E_INVALID: N, H, W < 1, cout not 32 | 64 | 128, C or cin outside 1 ... 4, slab_rows < 0, a null or unaligned (16 bytes; src
 *   of the pad: 4) pointer, dw and db both null, an unknown dtype code.  CPN_E_UNSUPPORTED: more than 2^31 - 1 pixels in Xq.
 *   CPN_E_WORKSPACE: a workspace smaller than cpn_image_conv_wgrad_workspace_bytes.  Every call validates before it reads a pointer.
 *
 * Saved for backward by image_conv2d: Xq alone (8 bytes per pixel, plus the border).  Known limits: no input gradient; the 1x1
 * shortcut and the ResBlock of ResUNet are not run; the norm's statistics are not folded into the epilogue; the conv's output is
 * saved by the norm behind it, not recomputed in the norm's backward; no fp8; the forward's stores are 32 contiguous bytes per
 * pixel and instruction (a pixel's line is completed by consecutive instructions of one wave).
 * ---------------------------------------------------------------------------------------------------------- */
int cpn_image_conv_pad(const float *src, int32_t N, int32_t C, int32_t H, int32_t W, void *xq, void *stream);
int cpn_image_conv_pack(const void *weight, int32_t weight_dtype, int32_t cout, int32_t cin, void *packed, void *stream);
int cpn_image_conv_forward(const void *xq, const void *packed, const float *bias, int32_t N, int32_t H, int32_t W, int32_t cout,
                           void *y, void *stream);
int cpn_image_conv_wgrad_info(int32_t N, int32_t H, int32_t W, int32_t cout, int32_t slab_rows, int32_t info[5]);
int64_t cpn_image_conv_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t cout, int32_t slab_rows);
int cpn_image_conv_wgrad(const void *xq, const void *dy, int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout,
                         int32_t slab_rows /* 0 = auto */, void *dw, int32_t dw_dtype, void *db, int32_t db_dtype, void *workspace,
                         int64_t workspace_bytes, void *stream);

/* ---- Trainable bilinear resize ------------------------------------------------------------------------------
 * What celldetection_amd.nn.bilinear_resize and nn.resized_conv2d need besides cpn_resize_bilinear, cpn_resize_bilinear_f32,
 * cpn_conv2d_sized and the "Trainable convolution" section to train the refinement head of a CPN: the resize of the refinement
 * features to the input's size in front of the head's k x k conv, and the resize of the head maps (csrc/bilinear_train.hip,
 * csrc/bilinear_adjoint.h, csrc/wgrad_dense.h, csrc/wgrad_slabs.h, csrc/wgrad_bias.h).  Additions to ABI 22.  This text is the
 * contract.
 *
 * The map.  B is F.interpolate(mode='bilinear', align_corners=False) from h x w to H x W, 1 <= h <= H, 1 <= w <= W.  Per axis,
 * output index dst reads
 *     f = fmaxf(scale * ((float) dst + 0.5f) - 0.5f, 0.f),  i0 = (int) f,  i1 = i0 + (i0 < in - 1),  lambda = f - (float) i0,
 *     scale = (float) in / (float) out,
 * as (1 - lambda) * src[i0] + lambda * src[i1]: the rule of bilinear_kernel, of the conv loader's halo_bilinear_store and of
 * resize_f32_kernel, restated as ba_tap in csrc/bilinear_adjoint.h.  The text leaves open how often the coordinate is rounded, and
 * the forward kernels differ in it: bilinear_kernel and the conv loader are compiled with contraction, which makes the product and
 * the difference ONE fma (the fused form: one rounding); resize_f32_kernel rounds each (the split form).  The forms agree where the
 * product is exact (the exact x2 among them) and differ by its rounding elsewhere (lambda by at most 2^-24 * in; where f falls on
 * an integer, the tap pair).  ba_tap states both, and every backward uses the form of ITS forward: fused for activations and for
 * the resized conv, split for the fp32 planes.  Everything after the coordinate is rounded to fp32 operation by operation (no
 * contraction).  Equal sizes make an axis the identity (f = dst, lambda = 0).  With hy = 1 - ly and hx = 1 - lx,
 *     B(x)[n][y][x] = hy * (hx * x[y0][x0] + lx * x[y0][x1]) + ly * (hx * x[y1][x0] + lx * x[y1][x1]).
 * i0 is non-decreasing in dst, so the outputs that touch source index i, those with i0 in {i - 1, i}, are one contiguous range
 * [ba_first(i - 1), ba_first(i + 1)), never empty; every output lies in two such ranges per axis, in one at the clamped last
 * index.  ba_weight(dst, i) = (i == i0) * (1 - lambda) + (i == i1) * lambda: at the clamped last index both terms apply.
 *
 * The adjoint.  For T at H x W, B^T(T)[n][i][j][c] = the sum over the footprint of (i, j) -- rows [ba_first(i - 1), ba_first(i + 1))
 * times columns likewise, in ascending row-major (y, x) order -- of c(y, x) * T[n][y][x][c] with the coefficient
 * c = ba_weight(y, i) * ba_weight(x, j) formed first (one fp32 product), then one multiply and one add per term, no fma, all in
 * fp32.  A gather: no floating-point atomics, no scatter, bit-identical from run to run.  At the exact x2 a footprint is
 * 4 x 4 (5 wide at source index 1, which the clamp at 0 gives a third output of index 0).
 *   cpn_bilinear_sum: bf16 NHWC T [N][H][W][C] -> bf16 [N][h][w][C], one rounding (RNE).  16 bytes (8 channels) per lane; C a
 *   positive multiple of 8, N, H, W >= 1, 1 <= h <= H, 1 <= w <= W (CPN_E_INVALID otherwise), N * H * W <= 2^31 - 1
 *   (CPN_E_UNSUPPORTED above), t and dst 16-byte aligned.
 *   cpn_bilinear_sum_f32: fp32 planes T [P][H][W] -> fp32 [P][h][w], the fp32 sum stored as it is; one lane per source pixel of one
 *   plane; the same checks with P in place of N, 4-byte alignment.  The backward of cpn_resize_bilinear_f32, whose taps are the same
 *   (its blend adds the column pair first: (v00 * hx + v01 * lx) * hy + (v10 * hx + v11 * lx) * ly).
 * Every call validates before it reads a pointer.
 *
 * The resized convolution.  y = conv(B(x), w) + b with x [N][h][w][cin] bf16 NHWC, w [cout][cin][k][k], k in {3, 5, 7}, stride 1,
 * padding k / 2 with zeros, cin and cout positive multiples of 32.  B(x) is never written.
 * Forward: cpn_conv2d_sized with up0 = 2 and stored = {h, w, ...} on the forward pack of w: the loader blends (MODE_BL of
 * csrc/conv_igemm.hip; compiled with contraction, so its blend may differ from the stated one in the last fp32 bit before the
 * rounding to bf16).
 * Input gradient: T = the dgrad conv of dY at H x W (bf16, "Trainable convolution"), then dx = B^T(T) by cpn_bilinear_sum.
 * Weight and bias gradients: dw[co][ci][ky][kx] = sum over pixels p of dY[p][co] * X[p + (ky - pad) * W + (kx - pad)][ci] with zeros
 * outside the image, where X = bf16(B(x)): the blend above in fp32 on the bf16 x, rounded to bf16 (RNE) when it is staged.
 * Partition, chains and rounding are those of cpn_conv_wgrad: slabs of slab_rows image rows of the N * H rows, 16 pixels per MFMA
 * step in one fp32 accumulator per output, then the slabs' partial sums added in ascending slab order (+ one add per slab), rounded
 * once to dw_dtype; db likewise from dY alone.  No floating-point atomics: bit-identical from run to run.  The four source pixels
 * (negative outside the tensor) and the two lambdas of each staged row are computed once per 128-pixel chunk into an LDS table;
 * every 16-byte item loads its four source items and blends.
 *   cpn_resized_conv_wgrad_info / cpn_resized_conv_wgrad_workspace_bytes / cpn_resized_conv_wgrad: the argument order of
 *   cpn_conv_wgrad_info / _workspace_bytes / cpn_conv_wgrad with (cin, h, w) in place of cin; H x W is the size of dY.  info[5] =
 *   {slabs, slab_rows, MFMA steps of the largest slab, reduce chain, bias chain}; the chain of one dw element is info[2] + 2 +
 *   info[3].  info and workspace_bytes answer without a GPU.  CPN_E_INVALID: N, H, W < 1, h / w outside 1 ... H / 1 ... W, cin or
 *   cout not positive multiples of 32, k not in {3, 5, 7}, slab_rows < 0, a null or unaligned (16 bytes) pointer, dw and db both
 *   null, an unknown dtype code.  CPN_E_UNSUPPORTED: more than 2^31 - 1 pixels or weights, more than 65535 tiles of 64 x 64
 *   channels, a chain longer than 2^31 - 1.  CPN_E_WORKSPACE: a workspace smaller than cpn_resized_conv_wgrad_workspace_bytes =
 *   slabs * (cin * cout * k * k + cout) * 4.  Every call validates before it reads a pointer.
 *
 * Saved for backward: by bilinear_resize the sizes alone, by resized_conv2d x at its low resolution (bf16) and w.  Known limits: T
 * is written and read once (no footprint sum in the dgrad epilogue); the forward is not decomposed into sub-pixel phases here; the
 * footprint sums walk a footprint serially in one lane, so a tiny source under a large map (h = w = 1 at the extreme) leaves a
 * handful of lanes reading the whole image: correct at any ratio, fast at the small ratios of a head; upward resizes only; no
 * bicubic; no 1 x 1 conv behind a resize.
 * ---------------------------------------------------------------------------------------------------------- */
int64_t cpn_resized_conv_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t cin, int32_t h, int32_t w, int32_t cout,
                                               int32_t k, int32_t slab_rows);
int cpn_resized_conv_wgrad_info(int32_t N, int32_t H, int32_t W, int32_t cin, int32_t h, int32_t w, int32_t cout, int32_t k,
                                int32_t slab_rows, int32_t info[5]);
int cpn_resized_conv_wgrad(const void *x, const void *dy, int32_t N, int32_t H, int32_t W, int32_t cin, int32_t h, int32_t w,
                           int32_t cout, int32_t k, int32_t slab_rows /* 0 = auto */, void *dw, int32_t dw_dtype, void *db,
                           int32_t db_dtype, void *workspace, int64_t workspace_bytes, void *stream);
int cpn_bilinear_sum(const void *t, int32_t N, int32_t H, int32_t W, int32_t C, void *dst, int32_t h, int32_t w, void *stream);
int cpn_bilinear_sum_f32(const float *t, int64_t planes, int32_t H, int32_t W, float *dst, int32_t h, int32_t w, void *stream);

/* ---- Augmentation warp --------------------------------------------------------------------------------------
 * What celldetection_amd.augment (warp, RandomAffine) runs on: one launch that warps a batch of channels-last images and their
 * [H, W, C] label stacks together, every sample by its own affine map, into the model's input layout and the label layout of
 * celldetection_amd.relabel_ and celldetection_amd.CPNTargetGenerator.feed (csrc/augment.hip, csrc/warp_rule.h).  It stands for the
 * albumentations pipeline of the reference's training recipe (Transpose, RandomRotate90, rotations and scalings, random crops,
 * RandomGamma / RandomBrightnessContrast, normalisation; celldetection/data/misc.py random_crop).  albumentations and
 * cv2.warpAffine are third-party, unpinned and absent here: their documented behaviour is restated, and their fixed-point
 * interpolation tables (cv2's 5-bit coordinate fraction and 15-bit weights) are deliberately NOT copied.  The independent anchor is
 * torch's float64 CPU grid_sample(align_corners=True), whose convention this is.  An addition to ABI 22.  This text is the contract.
 *
 * Coordinates.  Pixel centres lie at integer coordinates.  The map of a sample is six fp64 numbers m0 ... m5 that take a
 * DESTINATION pixel to a SOURCE position: for destination row i and column j, each converted exactly to double,
 *     sx = (m0 * j + m1 * i) + m2,      sy = (m3 * j + m4 * i) + m5,
 * every operation rounded to fp64, no contraction (the unit is compiled with -ffp-contract=off).
 *
 * Labels (nearest).  nx = floor(sx + 0.5), ny = floor(sy + 0.5) in fp64 (halves round up); the output is labels[ny][nx][c] for every
 * channel c, an int32 copied as it is: no value ever passes through a float, so negatives, -1 and 2^31 - 1 come out unchanged.
 *
 * Image (bilinear).  x0 = floor(sx), lx = (float) (sx - x0) (the difference is exact in fp64, one rounding to fp32), hx = 1.0f - lx;
 * likewise y0, ly, hy.  Each of the four taps (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1) is first mapped to fp32 by the
 * sample's intensity transform T (below): t00, t01, t10, t11.  Then
 *     out = (hy * (hx * t00 + lx * t01)) + (ly * (hx * t10 + lx * t11)),
 * every operation rounded to fp32, no fma: the order in which the bilinear kernels of this library blend.  A tap of weight 0 still
 * takes part (0 * t).
 *
 * Border: one mode per call, for taps and labels alike, applied per axis to the integer index.
 *   CPN_AUGMENT_BORDER_CONSTANT: a tap or label whose row or column lies outside the source is image_fill (a finite fp32, in the
 *   OUTPUT's units: it is not mapped by T) or label_fill.  Where all four taps of a pixel are outside, the output is image_fill
 *   itself (rounded to bf16 for a bf16 output), not the blend of four fills, whose fp32 weights need not sum to 1.
 *   CPN_AUGMENT_BORDER_REFLECT: reflect-101 indexing: p = 2 (n - 1), i <- i mod p (non-negative), i <- p - i where i >= n; n = 1: 0.
 * Range safety: indices are tested and reduced in fp64 BEFORE any conversion to an integer, so no map, NaN and infinities
 * included, forms an address outside the source.  An index further than 2^31 from the origin (or NaN) is outside the rule: it
 * counts as outside under CONSTANT and reads index 0 under REFLECT.  (The Python layer refuses such maps.)
 *
 * Intensity.  T is per sample and channel.
 *   CPN_AUGMENT_IMAGE_U8: a table of 256 fp32 entries, t = table[b][k][v].  Table-then-blend: a departure from albumentations, which
 *   blends the uint8 image, rounds to uint8 and then applies its tables; here nothing is rounded to uint8 in between.  The caller
 *   composes gamma, contrast, brightness, the scale to [0, 1] and the normalisation into the table in fp64 and rounds each entry
 *   once.  The kernel keeps the tables of its sample in LDS (K x 1 KiB).
 *   CPN_AUGMENT_IMAGE_F32: t = v * scale + offset with tables[b][k] = {scale, offset}, product and sum each rounded to fp32.
 *
 * Layouts.  image [B][H][W][K] (uint8 or fp32, channels-last as datasets hold images), labels [B][H][W][C] int32; image_out
 * [B][K][h][w] contiguous, out_dtype 0 (fp32) or 1 (bf16: one rounding to nearest even at the end), the codes of "Trainable
 * convolution"; labels_out [B][h][w][C] int32 contiguous.  All samples of a call share the source size.  Outputs must not overlap
 * inputs.  No atomics and no reductions: every output element is written exactly once, bit-identical from run to run.
 *
 * The launch.  One launch covers the batch: a workgroup of 256 lanes per CPN_AUGMENT_TILE x CPN_AUGMENT_TILE output tile and sample;
 * a lane computes four consecutive columns and writes each image plane with one 16-byte store (8 bytes for bf16) where w is a
 * multiple of 4 and image_out is aligned to it, element by element otherwise (the same values); the labels of a tile are copied
 * with one lane per (pixel, channel) in output order.
 *   cpn_augment_warp: image or labels may be null (a labels-only or image-only call: K, tables, image_fill, the dtypes and image_out,
 *   or C, label_fill and labels_out, are then not read).  CPN_E_INVALID: both null; B, H, W, h or w below 1; K outside 1 ... 4; C
 *   outside 1 ... CPN_AUGMENT_MAX_CHANNELS; an unknown dtype or border code; a non-finite image_fill; a null maps, tables or
 *   output of a part that is asked for; a pointer not aligned to its element (maps: 8 bytes).  CPN_E_UNSUPPORTED: 2^31 or more pixels
 *   in a source or a destination, more than 65535 samples or tile rows.  The call validates before it reads a pointer.
 * Known limits: no anti-aliasing when scaling down; affine maps only (no optical or elastic distortion, no blur, no noise);
 * table-then-blend; one source size per call; the four taps of a pixel are gathered from global memory, not staged in LDS.
 * ---------------------------------------------------------------------------------------------------------- */
#define CPN_AUGMENT_TILE 32
#define CPN_AUGMENT_MAX_CHANNELS 65535
#define CPN_AUGMENT_IMAGE_U8 0
#define CPN_AUGMENT_IMAGE_F32 1
#define CPN_AUGMENT_BORDER_CONSTANT 0
#define CPN_AUGMENT_BORDER_REFLECT 1
int cpn_augment_warp(const void *image, int32_t image_dtype /* u8 | f32 */, const int32_t *labels, int64_t B, int64_t H, int64_t W,
                     int32_t K, int32_t C, const double *maps /* [B][6], device */,
                     const float *tables /* u8: [B][K][256]; f32: [B][K][2]; device */, int32_t border, float image_fill,
                     int32_t label_fill, void *image_out, int32_t out_dtype /* f32 | bf16 */, int32_t *labels_out, int64_t h, int64_t w,
                     void *stream);

/* ---- Optimizer step -----------------------------------------------------------------------------------------
 * What celldetection_amd.optim (AdamW, clip_grad_norm_, grad_norm, step_info) runs on: the global L2 norm of a list of gradients,
 * the clip coefficient, the AdamW update and the in-place scaling of the gradients, each one multi-tensor launch
 * (csrc/optim.hip, csrc/optim_chunks.h).  They stand for torch.nn.utils.clip_grad_norm_ followed by torch.optim.AdamW.step, which
 * is what the reference trains with by default (models/lightning_base.py:397-400, dict(AdamW=dict()), under the trainer's gradient
 * clip).  Additions to ABI 22.  This text is the contract.
 *
 * The list.  n tensors; tensor t has numel[t] >= 0 contiguous elements of dtype 0 (fp32) or 1 (bf16), the codes of "Trainable
 * convolution".  Every tensor is cut on its own into chunks of CPN_OPTIM_CHUNK consecutive elements (the last one partial, a tensor
 * of 0 elements has none), tensor after tensor: chunk c of the list is chunk map[c][1] of tensor map[c][0].  The map is int32 [chunks][2]
 * and depends on the sizes alone.  One workgroup of 256 lanes takes one chunk at a time (at most 2048 workgroups, which walk more
 * chunks with that stride).  In a chunk, 16 bytes of the tensor's dtype (4 fp32 or 8 bf16 elements) are an item; item q belongs to
 * lane q % 256; a lane takes its items and the elements of an item in ascending order.  A lane moves a whole item with 16-byte
 * loads and stores (the fp32 state of 8 bf16 elements: two each) and the partial last item of a tensor element by element.  A
 * tensor one of whose addresses is not 16-byte aligned (CPN_OPTIM_FLAG_SCALAR, set by cpn_optim_upload) moves every item
 * element by element: the same lanes, the same order, the same results.
 *
 * The table.  CpnOptimTensor[n] in device memory, 8-byte aligned, one record per tensor: the four addresses, the size, the dtype
 * of p and g (m and v are fp32 whatever it is) and the fp32 scalars of the update, which the caller computes in fp64 and rounds
 * once:
 *     decay = 1 - lr * weight_decay,  w1 = 1 - beta1,  beta2,  w2 = 1 - beta2,  eps,  step_size = lr / (1 - beta1^t),
 *     bc2_sqrt = sqrt(1 - beta2^t),   t = the step count of the tensor after this step (>= 1).
 * (lr itself is carried for the record; the kernels do not read it.)  Steps and hyper-parameters may differ from tensor to tensor.
 *   cpn_optim_upload: validates a host table (pinned memory, or the copy is not asynchronous), writes every record's flags
 *   (CPN_OPTIM_FLAG_SCALAR where (p | g | m | v) & 15, opt_flags of csrc/optim_chunks.h; with_state = 0 clears p, m, v first: the
 *   norm and the scaling read g alone) and enqueues ONE hipMemcpyAsync of n records to `device` on the stream.  The host table
 *   must stay unchanged until that copy has run (the caller's ring of staging buffers).  CPN_E_INVALID: a negative size, an
 *   unknown dtype, a null address of a non-empty tensor, an address not aligned to its element.  n = 0 does nothing.
 *   cpn_optim_info: info[3] = {CPN_OPTIM_CHUNK, chunks, fp64 partials (= chunks)}; per_tensor (or NULL) int64 [n][3] =
 *   {first chunk, chunks, elements of the last chunk (0 for an empty tensor)}.  cpn_optim_chunk_map fills a host map of
 *   `chunks` records (CPN_E_INVALID where chunks is not the count of cpn_optim_info).  Host arithmetic: both answer without a GPU.
 *   More than 2^31 - 1 chunks: CPN_E_UNSUPPORTED.
 * A launch trusts no record of the map: one that names no tensor of the table, or a chunk past a tensor's end, is skipped, so
 * a map that does not fit the table can leave elements out and cannot reach outside a tensor.  cpn_optim_adamw skips a record
 * without p, m or v (a table uploaded with with_state = 0).
 *
 * The norm.  cpn_optim_sumsq writes one fp64 partial per chunk: a lane adds the squares of its elements, widened to fp64 (the
 * product is exact), in the order above; the 64 lanes of a wave are added by halving (lane l += lane l + 32, 16, 8, 4, 2, 1); the
 * four waves ((w0 + w1) + w2) + w3.  cpn_optim_norm (one workgroup): lane l adds partials [l * per, min(chunks, (l + 1) * per)),
 * per = ceil(chunks / 256), in ascending order, then the 256 lane sums are added in ascending order: S.  It writes
 *     norm_coef[0] = norm = (float) sqrt(S)                                   (fp64 square root, one rounding to fp32),
 *     norm_coef[1] = coef = (float) min(1, max_norm / ((double) norm + 1e-6))  (fp64, one rounding),
 * the clip_coef_clamped of torch.nn.utils.clip_grad_norm_; max_norm = +inf gives 1 (the norm alone), max_norm < 0 or NaN is
 * CPN_E_INVALID.  chunks = 0: norm 0.  No floating-point atomics: bit-identical from run to run.  A non-finite gradient gives a
 * non-finite norm, and a NaN coefficient stays NaN; nothing is skipped.
 *
 * The update.  cpn_optim_adamw, per element, every operation one fp32 operation rounded to nearest (no fma; IEEE division and
 * square root), in the order of torch's single-tensor path (torch/optim/adam.py _single_tensor_adam with decoupled decay):
 *     g = g * coef                        (coef = *coef, the word cpn_optim_norm wrote; coef == NULL: 1, and g * 1 is g)
 *     p = p * decay
 *     m = m + (g - m) * w1
 *     v = v * beta2 + (g * g) * w2
 *     denom = sqrt(v) / bc2_sqrt + eps
 *     p = p - step_size * (m / denom)
 * bf16 p and g widen exactly; the new p is rounded once to bf16 (to nearest even).  g is not written.  nontemporal = 1 stores m
 * and v with the non-temporal hint (same results; profiles/optim.txt says which is faster).
 * cpn_optim_scale: g = g * coef rounded once to g's dtype (for bf16 the product is formed exactly in fp64 first), in place: the
 * gradient scaling of clip_grad_norm_.
 * Every call validates before it reads a pointer; chunks = 0 launches nothing.
 * Known limits: not captured into a hipGraph by the caller (the table is uploaded per step); no fp32 master copy of a bf16
 * parameter; no skipping of a step on a non-finite norm; one workgroup per chunk, so a list of tiny tensors runs mostly idle lanes.
 * ---------------------------------------------------------------------------------------------------------- */
#define CPN_OPTIM_CHUNK 8192
#define CPN_OPTIM_FLAG_SCALAR 1
typedef struct CpnOptimTensor {
    void *p;         /* parameter, dtype below (unused by the norm and the scaling) */
    void *g;         /* gradient, the same dtype */
    float *m, *v;    /* exp_avg, exp_avg_sq */
    int64_t numel;
    int32_t dtype;   /* 0 fp32, 1 bf16 */
    int32_t flags;   /* written by the upload */
    float lr, decay, w1, beta2, w2, eps, step_size, bc2_sqrt;
} CpnOptimTensor;    /* 80 bytes */
int cpn_optim_info(CPN_HOST const int64_t *numel, int32_t n, int64_t info[3], CPN_HOST int64_t *per_tensor);
int cpn_optim_chunk_map(CPN_HOST const int64_t *numel, int32_t n, int32_t *map, int64_t chunks);
int cpn_optim_upload(CpnOptimTensor *host, int32_t n, int32_t with_state, void *device, void *stream);
int cpn_optim_sumsq(const void *table, int32_t n, const int32_t *map, int64_t chunks, double *partials, void *stream);
int cpn_optim_norm(const double *partials, int64_t chunks, double max_norm, float *norm_coef, void *stream);
int cpn_optim_adamw(const void *table, int32_t n, const int32_t *map, int64_t chunks, const float *coef, int32_t nontemporal,
                    void *stream);
int cpn_optim_scale(const void *table, int32_t n, const int32_t *map, int64_t chunks, const float *coef, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CPN_HIP_H */
