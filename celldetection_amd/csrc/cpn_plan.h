// Internal header of the native graph executor (include/cpn_hip.h is the public one).  The executor's host code is four units:
//   plan_validate.hip  validate_plan: every rule a descriptor array must satisfy + the record of its fused units
//   plan_shapes.hip    per-input-size planning: tensor sizes, which alternative of a unit runs, arena placement
//   conv_args.hip      ConvArgs / PairArgs from a descriptor (the plan's ops and the stand-alone entry points alike)
//   cpn_abi.hip        error state, the extern "C" surface and run_or_count (the one place that launches)
#pragma once
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/cpn_hip.h"
#include "cpn_error.h"
#include "cpn_kernels.h"

namespace cpn {

// A fused unit is three consecutive ops of which either the first or the other two run at a given input size (sub-pixel triples:
// head | phase + lateral) or either the first two or the third (c1 + c2 | the pair / bridge op that restates them).  validate_plan
// is the one place that establishes the positions; everything else goes through this record.
enum UnitRole : char {
    UNIT_NONE, UNIT_HEAD, UNIT_PHASE, UNIT_LATERAL, UNIT_BL_HEAD, UNIT_BL_PHASE, UNIT_BL_FRAME, UNIT_C1, UNIT_C2, UNIT_PAIR, UNIT_BRIDGE
};
struct OpUnit {
    UnitRole role = UNIT_NONE;
    int first = -1;  // index of the unit's first op
    int head() const { return first; }
    int phase() const { return first + 1; }
    int lateral() const { return first + 2; }  // (BL triples: the frame conv)
    int c1() const { return first; }
    int c2() const { return first + 1; }
    int fused() const { return first + 2; }
};

// The executor's A/B switches (kernel comparisons and tests), read from the environment when a shape is planned
struct Switches {
    int blphase = 1;  // CPN_BLPHASE: 0 never | 1 where it saves MACs | 2 wherever the resize is an exact x2
    int pair = 1;     // CPN_PAIR:    0 never | 1 where the launch fills the chip | 2 wherever supported
    int bridge = 1;   // CPN_BRIDGE:  0 never | 1 wherever the kernel's tiles fit
};
Switches read_switches();

// per conv op: what propagate_dims derived for it at this input size
struct ConvDims {
    int hin = 0, win = 0;  // virtual (post-resize) input size
    int stored[6] = {};    // stored sizes {Hs0, Ws0, Hs1, Ws1, Hr, Wr} of the two sources and the residual (0: absent)
};

struct ShapePlan {
    std::vector<int64_t> offsets;  // per tensor (arena byte offsets)
    std::vector<int> th, tw;       // per tensor spatial size for this input size (propagated op by op: any H x W)
    std::vector<char> skip;        // per op: not executed at this input size (the alternative of a fused unit / of the stem)
    std::vector<int> ring;         // per op: bilinear resize ops that write only a border ring of their output (0: whole map)
    std::vector<ConvDims> conv;    // per op (CPN_OP_CONV / CPN_OP_CONV_DEFERRED only)
    int out_h[CPN_NUM_OUTPUTS], out_w[CPN_NUM_OUTPUTS];  // sizes of the external fp32 outputs (0 = absent)
    int64_t total = 0;
    int64_t max_elems = 0;         // largest tensor of the graph, elements per image
    int error = 0;                 // CPN_E_* when the graph cannot run at this input size
    std::string message;
};

}  // namespace cpn

struct cpn_plan {
    std::vector<cpn_tensor_desc> tensors;
    std::vector<cpn_op_desc> ops;
    std::vector<cpn::OpUnit> units;  // per op (validate_plan)
    const unsigned char *weights = nullptr;
    size_t weight_bytes = 0;
    const float *bias = nullptr;
    size_t bias_count = 0;
    int precision = 0;  // CPN_PRECISION_BF16 / CPN_PRECISION_F32 / CPN_PRECISION_FP8
    // key: N, H, W, Switches.  Guarded by shape_mutex (std::map nodes are stable: returned references stay valid)
    std::map<std::tuple<int, int, int, int, int, int>, cpn::ShapePlan> shape_plans;
    std::mutex shape_mutex;
};

namespace cpn {

// 0, or CPN_E_* with the message recorded; fills plan.units
int validate_plan(cpn_plan &plan);

const ShapePlan &get_shape_plan(cpn_plan *p, int N, int H, int W);

// What a conv's argument building needs beyond its descriptor: the blobs its offsets index and the facts of the precision
struct ConvBinding {
    const void *weights = nullptr;  // weight_offset / fuse_weight_offset index this blob
    const float *bias = nullptr;    // bias_offset / fuse_bias_offset index this one (null: no bias)
    const float *mult = nullptr;    // fp8: this op's multipliers, resolved by the caller
    int record = 32;                // input channels per packed weight record: 32 | 64
    bool f32 = false;               // fp32 verification path
    float res_scale = 0.f, out_inv_scale = 0.f;  // fp8
    int res_wide = 0, dst_wide = 0;              // fp8 plans: bf16 partial sums of a sub-pixel triple
};
ConvBinding plan_binding(const cpn_plan &p, const cpn_op_desc &o);

// Hin x Win: virtual (post-resize) input size.  stored (optional): stored sizes {Hs0, Ws0, Hs1, Ws1, Hr, Wr} of the
// two sources and the residual; without it a resized source / residual is an exact x2 (the stand-alone cpn_conv2d).
int build_conv_args(const ConvBinding &b, const cpn_op_desc &o, int N, ConvArgs &a, const void *s0, int c0s, const void *s1, int c1s,
                    const void *res, int rs, void *dst, int ds, int Hin, int Win, const int *stored = nullptr);
// ConvArgs of a CPN_OP_CONV_BRIDGE op `o` (behind the scatter conv and the 3x3 conv c2 it restates) over an Hp x Wp source
int bridge_args(const ConvBinding &b, const cpn_op_desc &o, const cpn_op_desc &c2, int N, int Hp, int Wp, ConvArgs &a, const void *src,
                int c_stride, const void *res, int rs, void *dst, int ds);
double bridge_executed_flops(const ConvArgs &a);
// argument struct of a CPN_OP_CONV_PAIR op over an H x W source (tensor pointers filled by the caller)
PairArgs pair_args(const cpn_op_desc &o, int N, int H, int W, int c_stride, int dst_stride, const void *weights, const float *bias);
PairArgs plan_pair_args(const cpn_plan &p, const cpn_op_desc &o, int N, int H, int W);

}  // namespace cpn
