// Per-input-size planning of a validated plan: tensor sizes, which alternative of every fused unit runs, and the placement of the
// activations in the caller's arena (liveness-based first fit; static workspace planning instead of a caching allocator).
#include <algorithm>
#include <cstdlib>

#include "cpn_plan.h"

namespace cpn {

Switches read_switches() {
    Switches s;
    if (const char *e = getenv("CPN_BLPHASE")) s.blphase = atoi(e);
    if (const char *e = getenv("CPN_PAIR")) s.pair = atoi(e);
    if (const char *e = getenv("CPN_BRIDGE")) s.bridge = atoi(e) != 0;
    return s;
}

static int64_t tensor_bytes(const cpn_tensor_desc &t, int N, int h, int w, int elem) {
    const int64_t b = (int64_t) N * h * w * t.channels * elem;
    return (b + 255) / 256 * 256;
}

// Spatial sizes of every tensor for an H x W input, following the reference's modules: conv / max-pool output
// size = floor((in + 2p - k) / s) + 1; a nearest-resized source takes the size of the other concat source
// (F.interpolate(size=lateral.shape), models/unet.py:213-217, torchvision FPN) or, without one, twice its own size
// (scale_factor=2, bridge levels); CPN_OP_BILINEAR resizes to the INPUT size (_equal_size(features, inputs),
// models/cpn.py:277-278) and is a no-op alias when the sizes already agree.  (validate_plan has checked every tensor id, output
// index and divisor used here.)
static void propagate_dims(const cpn_plan *p, int N, int H, int W, ShapePlan &sp, const Switches &sw) {
    const int nt = (int) p->tensors.size();
    sp.th.assign(nt, 0);
    sp.tw.assign(nt, 0);
    for (int i = 0; i < CPN_NUM_OUTPUTS; ++i) sp.out_h[i] = sp.out_w[i] = 0;
    auto bad = [&](const char *m) { sp.error = CPN_E_INVALID; sp.message = m; };
    sp.skip.assign(p->ops.size(), 0);
    sp.ring.assign(p->ops.size(), 0);
    sp.conv.assign(p->ops.size(), ConvDims{});
    for (size_t oi = 0; oi < p->ops.size(); ++oi) {
        const cpn_op_desc &o = p->ops[oi];
        const OpUnit &u = p->units[oi];
        if (sp.error) return;
        if (u.role == UNIT_HEAD) {
            // the decomposition holds for the exact x2 case only (PyTorch's nearest index at any other ratio does not
            // split into phases): decided per input size
            const bool exact = p->precision != CPN_PRECISION_F32 && o.src1 >= 0 && o.up1 &&
                               sp.th[o.src0] == 2 * sp.th[o.src1] && sp.tw[o.src0] == 2 * sp.tw[o.src1];
            sp.skip[u.head()] = exact;
            sp.skip[u.phase()] = sp.skip[u.lateral()] = !exact;
        }
        if (u.role == UNIT_BL_HEAD) {
            // bilinear phases + frame instead of the conv over the resized map wherever the resize is an exact x2
            // ... and the decomposition executes fewer MACs than the conv it replaces: the frame is whole 8 x 32 tiles of the
            // k x k conv, most of a small image (CPN_BLPHASE=0 / 2: never / wherever exact -- kernel A/B and tests)
            // bf16 plans: head and frame conv resize their source in the halo loader (up0 == 2, all three ops read the
            // low-resolution map); fp8 plans: the resize is an op of its own, head and frame conv read its output
            const int lo = p->ops[u.phase()].src0;
            const bool hi_ok = o.up0 == 2 ? lo == o.src0 : (sp.th[o.src0] == H && sp.tw[o.src0] == W);
            bool exact = sw.blphase != 0 && p->precision != CPN_PRECISION_F32 && hi_ok && 2 * sp.th[lo] == H && 2 * sp.tw[lo] == W &&
                         sp.th[lo] >= o.kh && sp.tw[lo] >= o.kw;
            if (exact && sw.blphase != 2) {
                const int k2 = (o.kh + 3) / 2, m = 2 * ((o.kh / 2 + 1) / 2);
                auto tiles = [](int h, int w) { return (double) ((h + 7) / 8) * ((w + 31) / 32); };
                // frame tiles exactly as the frame launch enumerates them (cpn_kernels.h frame_tiles, 8 x 32 tiles of a stride-1
                // k x k conv: whole tile rows above / below the box, per row that crosses it one wrap tile or its side tiles)
                const double frame = (double) frame_tiles(H, W, m, 8, 32, o.kw > 1 ? o.kw : 0).total;
                const double head = tiles(H, W) * o.kh * o.kh;
                const double parts = 4. * tiles(H / 2, W / 2) * k2 * k2 + frame * o.kh * o.kh;
                exact = parts <= 0.85 * head;
            }
            if (exact && o.up0 != 2) {
                // the materialised resized map is read by the frame conv alone: its resize op writes only the pixels the
                // frame's outputs reach (frame width + conv padding from the border)
                int producer = -1;
                bool shared = false;
                for (int j = 0; j < (int) p->ops.size(); ++j) {
                    const cpn_op_desc &q = p->ops[j];
                    if (j < u.head() && q.op == CPN_OP_BILINEAR && q.dst == o.src0 && q.subpixel == CPN_SUBPIXEL_BL_FRAME) producer = j;
                    if (j != u.head() && j != u.lateral() && (q.src0 == o.src0 || q.src1 == o.src0 || q.res == o.src0)) shared = true;
                }
                if (producer >= 0 && !shared) sp.ring[producer] = 2 * ((o.kh / 2 + 1) / 2) + o.kh / 2;
            }
            sp.skip[u.head()] = exact;
            sp.skip[u.phase()] = sp.skip[u.lateral()] = !exact;
        }
        if (o.alt == 1 || o.alt == 2) {
            // stem alternatives: the fast pair (padded 4-channel input layout inside the input tensor's storage + the
            // dedicated 7x7 stride-2 kernel) wherever that layout fits, the generic pair otherwise
            int tin = -1;
            for (const cpn_op_desc &q : p->ops)
                if (q.op == CPN_OP_INPUT) { tin = q.dst; break; }
            // (the padded layout is bf16 [H + 6][W + 8][4] = 8 bytes per pixel in bf16 AND fp8 plans; the input tensor
            // offers channels * 2 | 1 bytes per pixel)
            const int elem = p->precision == CPN_PRECISION_FP8 ? 1 : 2;
            const bool fast = p->precision != CPN_PRECISION_F32 && tin >= 0 &&
                              (int64_t) (H + STEM_PAD_ROWS) * (W + STEM_PAD_COLS) * 8 <=
                                  (int64_t) H * W * p->tensors[tin].channels * elem;
            sp.skip[oi] = (o.alt == 2) != fast;
        }
        switch (o.op) {
            case CPN_OP_CONV_BRIDGE: {
                // runs instead of the scatter conv + 3x3 conv in front of it wherever the kernel's 16 x 32 tiles fit the output
                // (CPN_BRIDGE=0: never -- kernel A/B and tests)
                const int Hp = sp.th[o.src0], Wp = sp.tw[o.src0];
                const bool fused = sw.bridge != 0 && p->precision == CPN_PRECISION_BF16 && 2 * Hp >= 16 && 2 * Wp >= 32 &&
                                   sp.th[o.dst] == 2 * Hp && sp.tw[o.dst] == 2 * Wp;
                sp.skip[u.fused()] = !fused;
                sp.skip[u.c1()] = sp.skip[u.c2()] = fused;
                break;
            }
            case CPN_OP_CONV_PAIR: {
                // runs instead of the two convs in front of it wherever the kernel's full-width strips fit the feature map
                // and its strips x slabs fill the chip (CPN_PAIR=0 / 2: never / wherever supported -- kernel A/B and tests)
                const int mid = p->ops[u.c1()].dst;  // conv1's output: the kernel's H x W (conv2 may stride it down)
                const PairArgs pa = plan_pair_args(*p, o, N, sp.th[mid], sp.tw[mid]);
                const bool fused = sw.pair != 0 && p->precision == CPN_PRECISION_BF16 && conv_pair_supported(pa) &&
                                   (sw.pair == 2 || conv_pair_blocks(pa) >= 192);
                sp.skip[u.fused()] = !fused;
                sp.skip[u.c1()] = sp.skip[u.c2()] = fused;
                break;
            }
            case CPN_OP_INPUT:
            case CPN_OP_INPUT_STEM: sp.th[o.dst] = H; sp.tw[o.dst] = W; break;
            case CPN_OP_STEM7:
                sp.th[o.dst] = (sp.th[o.src0] - 1) / 2 + 1;  // floor((in + 6 - 7) / 2) + 1
                sp.tw[o.dst] = (sp.tw[o.src0] - 1) / 2 + 1;
                break;
            case CPN_OP_MAXPOOL:
                sp.th[o.dst] = (sp.th[o.src0] + 2 * o.pad - o.kh) / o.stride + 1;
                sp.tw[o.dst] = (sp.tw[o.src0] + 2 * o.pad - o.kw) / o.stride + 1;
                if (sp.th[o.src0] + 2 * o.pad < o.kh || sp.tw[o.src0] + 2 * o.pad < o.kw) bad("input too small for the max-pool");
                break;
            case CPN_OP_BILINEAR: sp.th[o.dst] = H; sp.tw[o.dst] = W; break;
            case CPN_OP_ACT: sp.th[o.dst] = sp.th[o.src0]; sp.tw[o.dst] = sp.tw[o.src0]; break;
            case CPN_OP_CONV:
            case CPN_OP_CONV_DEFERRED: {
                if (o.up0 && o.up1) { bad("conv: both sources resized"); break; }
                // the virtual input size, and the stored sizes the run hands to build_conv_args
                ConvDims &cd = sp.conv[oi];
                if (o.up0 == 2) { cd.hin = H; cd.win = W; }  // bilinear resize of the source to the INPUT size (cpn.py:277-278)
                else if (o.up1) { cd.hin = sp.th[o.src0]; cd.win = sp.tw[o.src0]; }
                else if (o.up0 && o.src1 >= 0) { cd.hin = sp.th[o.src1]; cd.win = sp.tw[o.src1]; }
                else if (o.up0) { cd.hin = 2 * sp.th[o.src0]; cd.win = 2 * sp.tw[o.src0]; }
                else { cd.hin = sp.th[o.src0]; cd.win = sp.tw[o.src0]; }
                cd.stored[0] = sp.th[o.src0]; cd.stored[1] = sp.tw[o.src0];
                if (o.src1 >= 0) { cd.stored[2] = sp.th[o.src1]; cd.stored[3] = sp.tw[o.src1]; }
                if (o.res >= 0) { cd.stored[4] = sp.th[o.res]; cd.stored[5] = sp.tw[o.res]; }
                const int hv = cd.hin, wv = cd.win;
                if (o.subpixel == CPN_SUBPIXEL_PHASE) {  // 2 x 2 taps per output phase: the output keeps the source's size
                    sp.th[o.dst] = sp.th[o.src0]; sp.tw[o.dst] = sp.tw[o.src0];
                    break;
                }
                if (o.subpixel == CPN_SUBPIXEL_BL_PHASE) break;  // (writes the BL_HEAD op's external output: sized there)
                if (o.subpixel == CPN_SUBPIXEL_SCATTER) {  // conv over the x2-upsampled source (scale_factor = 2)
                    if (o.dst < 0) { bad("conv: a sub-pixel scatter conv needs a tensor destination"); break; }
                    sp.th[o.dst] = 2 * sp.th[o.src0]; sp.tw[o.dst] = 2 * sp.tw[o.src0];
                    break;
                }
                if (!o.up0 && !o.up1 && o.src1 >= 0 && (sp.th[o.src1] != hv || sp.tw[o.src1] != wv)) { bad("conv: concat sources differ in size"); break; }
                if (hv + 2 * o.pad < o.kh || wv + 2 * o.pad < o.kw) { bad("input too small for a convolution of the graph"); break; }
                const int ho = (hv + 2 * o.pad - o.kh) / o.stride + 1, wo = (wv + 2 * o.pad - o.kw) / o.stride + 1;
                if (o.res >= 0 && !o.res_up && (sp.th[o.res] != ho || sp.tw[o.res] != wo)) { bad("conv: residual size mismatch"); break; }
                if (o.res >= 0 && o.res_up == 2 && !sp.skip[oi] && (2 * sp.th[o.res] != ho || 2 * sp.tw[o.res] != wo)) { bad("conv: phase tensor size mismatch"); break; }
                if (o.dst >= 0) { sp.th[o.dst] = ho; sp.tw[o.dst] = wo; }
                else { sp.out_h[o.out_index] = ho; sp.out_w[o.out_index] = wo; }
                break;
            }
            default: bad("unknown op");
        }
    }
    for (int t = 0; t < nt && !sp.error; ++t) {
        if (sp.th[t] < 0 || sp.tw[t] < 0) bad("negative tensor size");
        sp.max_elems = std::max(sp.max_elems, (int64_t) sp.th[t] * sp.tw[t] * p->tensors[t].channels);
    }
}

// Arena byte offsets of every tensor that is written at this input size: first fit over the tensors whose lifetimes overlap
static void place_arena(const cpn_plan *p, int N, ShapePlan &sp) {
    const int nt = (int) p->tensors.size();
    // a bilinear op whose source already has the input size is an alias (no kernel, shared storage)
    std::vector<int> root(nt);
    for (int t = 0; t < nt; ++t) root[t] = t;
    for (const cpn_op_desc &o : p->ops)
        if (o.op == CPN_OP_BILINEAR && sp.th[o.src0] == sp.th[o.dst] && sp.tw[o.src0] == sp.tw[o.dst]) root[o.dst] = root[o.src0];
    std::vector<int> def(nt, -1), last(nt, -1);
    for (int i = 0; i < (int) p->ops.size(); ++i) {
        const cpn_op_desc &o = p->ops[i];
        if (sp.skip[i]) continue;  // (the alternative of a fused unit that does not run at this size)
        if (o.dst >= 0 && def[root[o.dst]] < 0) def[root[o.dst]] = i;
        // (the sources of a deferred conv are read after the run, cpn_sparse_heads: they stay live to the end)
        const int use = o.op == CPN_OP_CONV_DEFERRED ? (int) p->ops.size() : i;
        for (int s_ : {o.src0, o.src1, o.res})
            if (s_ >= 0) last[root[s_]] = std::max(last[root[s_]], use);
        if (o.dst >= 0) last[root[o.dst]] = std::max(last[root[o.dst]], i);
    }
    std::vector<int> order;
    for (int t = 0; t < nt; ++t)
        if (root[t] == t && def[t] >= 0) order.push_back(t);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return def[a] < def[b]; });
    // bytes per element: fp32 4 | bf16 2 | e4m3 1 -- except the bf16 partial-sum tensors of an fp8 plan (scale < 0)
    auto elem_of = [&](int t) {
        return p->precision == CPN_PRECISION_F32 ? 4 : (p->precision == CPN_PRECISION_FP8 ? (p->tensors[t].scale < 0.f ? 2 : 1) : 2);
    };
    std::vector<int> placed;
    for (int t : order) {
        const int64_t sz = tensor_bytes(p->tensors[t], N, sp.th[t], sp.tw[t], elem_of(t));
        // candidate offsets: 0 and the end of every conflicting placed tensor; take the lowest that fits
        std::vector<std::pair<int64_t, int64_t>> busy;  // [begin, end) of live-overlapping tensors
        for (int q : placed)
            if (!(last[q] < def[t] || last[t] < def[q]))
                busy.emplace_back(sp.offsets[q], sp.offsets[q] + tensor_bytes(p->tensors[q], N, sp.th[q], sp.tw[q], elem_of(q)));
        std::sort(busy.begin(), busy.end());
        int64_t off = 0;
        for (auto &b : busy) {
            if (off + sz <= b.first) break;
            off = std::max(off, b.second);
        }
        sp.offsets[t] = off;
        sp.total = std::max(sp.total, off + sz);
        placed.push_back(t);
    }
    for (int t = 0; t < nt; ++t)
        if (root[t] != t) sp.offsets[t] = sp.offsets[root[t]];
}

const ShapePlan &get_shape_plan(cpn_plan *p, int N, int H, int W) {
    std::lock_guard<std::mutex> lock(p->shape_mutex);
    // the switches are part of the key: toggling one on a live plan re-plans the shape (the Python engine's hipGraph key carries
    // them as well)
    const Switches sw = read_switches();
    const auto key = std::make_tuple(N, H, W, sw.blphase, sw.pair, sw.bridge);
    auto it = p->shape_plans.find(key);
    if (it != p->shape_plans.end()) return it->second;
    ShapePlan sp;
    propagate_dims(p, N, H, W, sp, sw);
    sp.offsets.assign(p->tensors.size(), -1);
    if (!sp.error) place_arena(p, N, sp);
    return p->shape_plans.emplace(key, std::move(sp)).first->second;
}

}  // namespace cpn
