"""Builds libcpn_hip.so (hand-written HIP kernels + C ABI) in-tree for gfx950 with hipcc.

    python -m celldetection_amd.build [--force]

hipcc cross-compiles without a GPU; the resulting .so is git-ignored but travels with the repo snapshot to the
GPU box.  Only gfx950 (MI355X / CDNA4) is targeted -- no multi-arch, no compatibility paths.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
OUT = os.path.join(HERE, 'libcpn_hip.so')
OUT_CLOCK = os.path.join(HERE, 'libcpn_hip_clock.so')  # measurement variant: shader-clock probe in the bf16 conv kernels
ARCH = 'gfx950'

SOURCES = {
    # file: extra flags
    'conv_igemm.hip': [],
    'conv_fp8.hip': [],  # the same source with CPN_FP8 = 1 (e4m3 operands)
    'conv_pair.hip': [],
    'misc_kernels.hip': [],
    'misc_fp8.hip': [],
    'conv_f32.hip': [],
    # decode/NMS must reproduce the reference's fp32 operation order bit-for-bit: no FMA contraction
    'decode_nms.hip': ['-ffp-contract=off'],
    'nms_binned.hip': ['-ffp-contract=off'],
    'labels.hip': [],
    'instance_eval.hip': [],  # integer only
    'flat_labels.hip': [],  # integer only
    # integer accumulation; the fp64 finalisation is defined by its order of operations: no FMA contraction
    'region_props.hip': ['-ffp-contract=off'],
    # integer counts; the fp64 finalisation is defined by its order of operations: no FMA contraction
    'shape_props.hip': ['-ffp-contract=off'],
    # integer overlay sums; the float32 colour-map reduction is defined by its order of operations: separate multiply and add,
    # correctly rounded division
    'overlay.hip': ['-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt'],
    # integer components and border following; the fp64 resampling is defined by its order of operations: no FMA contraction
    # (fp64 sqrt and division are correctly rounded as they stand)
    'label_contours.hip': ['-ffp-contract=off'],
    # integer only: the components pass shared with label_contours.hip (csrc/components.h) and the numbering
    'components.hip': [],
    # fp64 sums whose result is defined by their order of operations (csrc/efd_chunks.h): no FMA contraction
    'contour_fourier.hip': ['-ffp-contract=off'],
    # integer chamfer relaxation; the float32 normalisation is one IEEE division per pixel: correctly rounded, no contraction
    'label_distances.hip': ['-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt'],
    # the training objective shares the decode's float32 arithmetic (decode_device.h) and defines its float64 sums and gradients
    # by their order of operations: no FMA contraction
    'cpn_objective.hip': ['-ffp-contract=off'],
    # trainable convolution: weight packing on the device and the MFMA weight gradient (slab partition: csrc/wgrad_slabs.h)
    'conv_train.hip': [],
    # trainable batch normalisation (+ ReLU): fp64 sums in a fixed order and named fp32 fmas (lane mapping: csrc/bn_slabs.h): no
    # FMA contraction
    'batch_norm.hip': ['-ffp-contract=off'],
    # trainable ReadOut tail: Dropout2d + 1x1 conv to few channels, three MFMA products (partition: csrc/tail_slabs.h)
    'readout_tail.hip': [],
    # trainable grouped 3x3 conv: block-diagonal packs, stride-2 dilation, the weight gradient of the diagonal fragments (index
    # arithmetic: csrc/grouped_conv.h; the slab kernel: csrc/wgrad_dense.h; the bias gradient's kernels: csrc/wgrad_bias.h)
    'grouped_conv_train.hip': [],
    # trainable concat conv of the decoder: the weight gradient over the virtual concat of the lateral and the nearest-resized top,
    # and the adjoint of the resize (index arithmetic: csrc/nearest_adjoint.h)
    'cat_conv_train.hip': [],
    # trainable bilinear resize of the refinement head: the adjoint of the resize as a gather (activations and fp32 planes) and the
    # weight gradient of a conv over the virtual resized tensor; the blend and the sums are defined by their order of operations
    # (index arithmetic: csrc/bilinear_adjoint.h): no FMA contraction
    'bilinear_train.hip': ['-ffp-contract=off'],
    # trainable ResNet stem (7x7 stride-2 conv on the padded 4-channel input: forward, weight gradient; what it shares with the image
    # conv: csrc/image_train.h)
    'stem_train.hip': [],
    # max-pool with its tap index and gather gradient (index arithmetic: csrc/pool_adjoint.h)
    'pool_train.hip': [],
    # trainable image conv (the 3x3 stride-1 first conv of the U-Net encoders on the padded 4-channel image: pad, forward, weight
    # gradient; pack, slab reduce, checks and host path: csrc/image_train.h)
    'image_conv_train.hip': [],
    # the optimizer step (global gradient norm, clip, AdamW): fp64 sums in a fixed order and an fp32 update defined operation by
    # operation (partition and lane mapping: csrc/optim_chunks.h): no FMA contraction, correctly rounded division and square root
    'optim.hip': ['-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt'],
    # training augmentation: the joint affine warp of image and labels; the fp64 position and the fp32 blend are defined by their
    # order of operations (index and weight arithmetic: csrc/warp_rule.h): no FMA contraction
    'augment.hip': ['-ffp-contract=off'],
    'sparse_heads.hip': [],
    'stem.hip': [],
    # the native graph executor (host code only; cpn_plan.h names the units)
    'plan_validate.hip': [],
    'plan_shapes.hip': [],
    'conv_args.hip': [],
    'cpn_abi.hip': [],
}
HEADERS = ['cpn_kernels.h', 'cpn_error.h', 'cpn_plan.h', 'lds_dma.h', 'polygon_fill.h', 'contour_trace.h', 'components.h', 'component_rank.h', 'wgrad_slabs.h', 'wgrad_bias.h', 'wgrad_dense.h', 'mfma_frag.h', 'stem_mfma.h', 'image_train.h', 'grouped_conv.h', 'nearest_adjoint.h', 'bilinear_adjoint.h', 'pool_adjoint.h', 'bn_slabs.h', 'tail_slabs.h', 'optim_chunks.h', 'warp_rule.h', 'efd_chunks.h', 'label_table.h', 'props_table.h', 'hull_count.h', 'decode_device.h', 'conv_igemm.hip', os.path.join('..', '..', 'include', 'cpn_hip.h')]


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if c and (os.path.isfile(c) or c == 'hipcc'):
            return c
    return 'hipcc'


def _stale(target, deps):
    if not os.path.isfile(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.isfile(d))


def build(force=False, verbose=True):
    objdir = os.path.join(HERE, 'build')
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    objs, procs = [], []
    for src, extra in SOURCES.items():
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace('.hip', '.o'))
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            cmd = [_hipcc(), f'--offload-arch={ARCH}', '-O3', '-std=c++17', '-fPIC', '-c', s, '-o', o] + extra + \
                  os.environ.get('CPN_HIPCC_FLAGS', '').split()
            if verbose:
                print(' '.join(cmd), flush=True)
            procs.append((src, subprocess.Popen(cmd)))
    for src, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f'hipcc failed on {src}')
    if force or procs or _stale(OUT, objs):
        cmd = [_hipcc(), f'--offload-arch={ARCH}', '-shared', '-fPIC'] + objs + ['-o', OUT]
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.check_call(cmd)
    # libcpn_hip_clock.so: the same library with the shader-clock probe compiled into the bf16 conv kernels
    # (include/cpn_hip.h cpn_debug_clock_probe; bench.py runs it in a child process next to the roofline numbers)
    s = os.path.join(CSRC, 'conv_igemm.hip')
    o = os.path.join(objdir, 'conv_igemm_clock.o')
    if force or _stale(o, [s] + hdrs):
        cmd = [_hipcc(), f'--offload-arch={ARCH}', '-O3', '-std=c++17', '-fPIC', '-c', s, '-o', o, '-DCPN_EXP_CLOCK=2'] + \
              os.environ.get('CPN_HIPCC_FLAGS', '').split()
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.check_call(cmd)
    cobjs = [o if x.endswith(os.sep + 'conv_igemm.o') else x for x in objs]
    if force or _stale(OUT_CLOCK, cobjs):
        cmd = [_hipcc(), f'--offload-arch={ARCH}', '-shared', '-fPIC'] + cobjs + ['-o', OUT_CLOCK]
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.check_call(cmd)
    return OUT


if __name__ == '__main__':
    print(build(force='--force' in sys.argv))
