"""One conv case per kernel instantiation (test data and helpers: no tests, not a conftest).

conv_igemm.hip compiles conv_igemm_kernel<TH, BN, WM, WN, MODE> for nine tiles x five plain modes (+ MODE_S1F, MODE_S1Q,
MODE_BR on one tile each) in the bf16 unit and nine tiles x three modes in the e4m3 unit (conv_fp8.hip).  Which one a call
runs is decided on the host (conv_mode, choose_tile, the fused-head override); the library answers that through
cpn_conv2d_kernel_info (celldetection_amd._lib.conv_kernel_info), the selection step of the launch itself.  Nothing here
restates the selection: every key below is what the LIBRARY says the case runs (tests/test_conv_tiles.py asserts it without
a GPU, tests/test_gpu_conv_tiles.py once more on the GPU machine before it runs the case).

Keys: '<unit>/<mode>/<TH>x<BN>[+<second epilogue>]', e.g. 'bf16/S1/8x256', 'e4m3/PW/16x64', 'bf16/PW/8x256+res_up'.
Values: the keyword arguments of test_gpu_kernels.run_conv (bf16) or run_conv_fp8 (e4m3); ENV: switches a case is run under;
'bf16/BR/16x64' names a case of tests/test_gpu_conv_bridge.py.

Every entry is the cheapest shape of a search over n, h, w and cout, driven through the library's query, that shows for the
tile it runs (edges(): computed from the shape and the tile the library returned):

  n2      N >= 2
  row     a partial last row tile: Hout % TH != 0 (MODE_N: of the virtual Hout / 2 rows of 32 pixels)
  col     a partial last column tile: Wout % 32 != 0 (MODE_N: not applicable, the width is 16)
  full    a tile with TH full rows and 32 full columns as well (the epilogue's full_tile fast path; BN <= cout_b always, so
          its first channel block is full, too)
  cblk    a partial last channel block: cout_b % BN != 0 (not applicable at BN = 32 and to fused heads, whose block owns
          every channel)
  cpad    a real cout that is no multiple of 32: the padded channels must come back zero (checked on NHWC outputs; fp32 NCHW
          outputs hold the real planes only, their guard bands are checked instead)
  chunks  at least two K chunks (32 channels bf16, 64 e4m3)
  odd     an odd packed item count (chunks x taps): the zero slab that pads it is read

EXEMPT lists the edges an entry cannot show, each with its reason.  cin = 96 (bf16) / 192 (e4m3): three chunks, 27 items
of a 3x3.  The fill threshold of choose_tile (224 blocks, 448 for the 16-row tile) forces the batch sizes: 8-row tiles need
N = 28 with 2 x 2 spatial tiles and two channel blocks, the 16-row tile and the single-block 8x32 tiles N = 56 (MODE_N: one
tile per row pair, so twice that).

Second epilogues (+res: residual, +res_up: x2 nearest-resized residual, +concat_up: second source read through nearest x2,
+f32: fp32 NCHW output, +fused: fused ReadOut tail) are entered on one big and one small tile of each mode that has them.
e4m3: NHWC outputs are padded to 64 channels, so BN = 32 exists for fp32 / fused outputs only (cout_b = 32) and a partial
last block at BN = 64 for fp32 outputs only (cout_b = 96): the 64-channel tiles at 4 and 8 rows have an NHWC entry and a +f32
entry, the 16-row tile (448 blocks) the fp32 one.
"""
import contextlib
import os
import re
import struct

EDGES = ('n2', 'row', 'col', 'full', 'cblk', 'cpad', 'chunks', 'odd')

TABLE = {
    'bf16/PW/16x64': dict(n=56, h=17, w=33, cin=96, cout=88, k=1),
    'bf16/PW/8x256': dict(n=28, h=9, w=33, cin=96, cout=280, k=1),
    'bf16/PW/8x256+f32': dict(n=28, h=9, w=33, cin=96, cout=280, k=1, out_f32=True, bn=False, act='sigmoid'),
    'bf16/PW/8x256+res': dict(n=28, h=9, w=33, cin=96, cout=280, k=1, res=True),
    'bf16/PW/8x256+res_up': dict(n=28, h=9, w=33, cin=96, cout=280, k=1, res=True, res_up=True),
    'bf16/PW/8x128': dict(n=28, h=9, w=33, cin=96, cout=136, k=1),
    'bf16/PW/8x64': dict(n=28, h=9, w=33, cin=96, cout=88, k=1),
    'bf16/PW/8x32': dict(n=56, h=9, w=33, cin=96, cout=24, k=1),
    'bf16/PW/4x256': dict(n=28, h=5, w=33, cin=96, cout=280, k=1),
    'bf16/PW/4x128': dict(n=28, h=5, w=33, cin=96, cout=136, k=1),
    'bf16/PW/4x64': dict(n=2, h=5, w=33, cin=96, cout=88, k=1),
    'bf16/PW/4x64+res': dict(n=2, h=5, w=33, cin=96, cout=88, k=1, res=True),
    'bf16/PW/4x64+res_up': dict(n=2, h=5, w=33, cin=96, cout=88, k=1, res=True, res_up=True),
    'bf16/PW/4x32': dict(n=2, h=5, w=33, cin=96, cout=24, k=1),
    'bf16/PW/4x32+f32': dict(n=2, h=5, w=33, cin=96, cout=24, k=1, out_f32=True, bn=False, act='sigmoid'),
    'bf16/S1/16x64': dict(n=56, h=17, w=33, cin=96, cout=88, k=3),
    'bf16/S1/8x256': dict(n=28, h=9, w=33, cin=96, cout=280, k=3),
    'bf16/S1/8x256+concat_up': dict(n=28, h=9, w=33, cin=96, cout=280, k=3, cin1=64, up1=True),
    'bf16/S1/8x256+f32': dict(n=28, h=9, w=33, cin=96, cout=280, k=3, out_f32=True, bn=False, act='tanh_scaled'),
    'bf16/S1/8x256+fused': dict(n=2, h=9, w=33, cin=96, cout=250, k=3, fuse_cout=20, fuse_act='none'),
    'bf16/S1/8x256+res': dict(n=28, h=9, w=33, cin=96, cout=280, k=3, res=True),
    'bf16/S1/8x128': dict(n=28, h=9, w=33, cin=96, cout=136, k=3),
    'bf16/S1/8x64': dict(n=28, h=9, w=33, cin=96, cout=88, k=3),
    'bf16/S1/8x32': dict(n=56, h=9, w=33, cin=96, cout=24, k=3),
    'bf16/S1/8x32+fused': dict(n=2, h=9, w=33, cin=96, cout=24, k=3, fuse_cout=20, fuse_act='none'),
    'bf16/S1/4x256': dict(n=28, h=5, w=33, cin=96, cout=280, k=3),
    'bf16/S1/4x128': dict(n=28, h=5, w=33, cin=96, cout=136, k=3),
    'bf16/S1/4x64': dict(n=2, h=5, w=33, cin=96, cout=88, k=3),
    'bf16/S1/4x64+concat_up': dict(n=2, h=5, w=33, cin=96, cout=88, k=3, cin1=64, up1=True),
    'bf16/S1/4x64+res': dict(n=2, h=5, w=33, cin=96, cout=88, k=3, res=True),
    'bf16/S1/4x32': dict(n=2, h=5, w=33, cin=96, cout=24, k=3),
    'bf16/S1/4x32+f32': dict(n=2, h=5, w=33, cin=96, cout=24, k=3, out_f32=True, bn=False, act='tanh_scaled'),
    'bf16/S2/8x256': dict(n=28, h=17, w=65, cin=32, cout=280, k=3, stride=2),
    'bf16/S2/8x128': dict(n=28, h=17, w=65, cin=32, cout=136, k=3, stride=2),
    'bf16/S2/8x64': dict(n=28, h=17, w=65, cin=32, cout=88, k=3, stride=2),
    'bf16/S2/8x32': dict(n=56, h=17, w=65, cin=32, cout=24, k=3, stride=2),
    'bf16/S2/4x256': dict(n=28, h=9, w=65, cin=96, cout=280, k=3, stride=2),
    'bf16/S2/4x256+res': dict(n=28, h=9, w=65, cin=96, cout=280, k=3, stride=2, res=True),
    'bf16/S2/4x128': dict(n=28, h=9, w=65, cin=96, cout=136, k=3, stride=2),
    'bf16/S2/4x64': dict(n=2, h=9, w=65, cin=96, cout=88, k=3, stride=2),
    'bf16/S2/4x64+res': dict(n=2, h=9, w=65, cin=96, cout=88, k=3, stride=2, res=True),
    'bf16/S2/4x32': dict(n=2, h=9, w=65, cin=96, cout=24, k=3, stride=2),
    'bf16/BL/16x64': dict(n=56, h=17, w=33, cin=96, cout=88, k=3, bilinear=True),
    'bf16/BL/8x256': dict(n=28, h=9, w=33, cin=96, cout=280, k=3, bilinear=True),
    'bf16/BL/8x256+f32': dict(n=28, h=9, w=33, cin=96, cout=280, k=3, bilinear=True, out_f32=True, bn=False, act='none'),
    'bf16/BL/8x256+fused': dict(n=2, h=9, w=33, cin=96, cout=250, k=3, bilinear=True, fuse_cout=2, fuse_act='tanh_scaled'),
    'bf16/BL/8x256+res': dict(n=28, h=9, w=33, cin=96, cout=280, k=3, bilinear=True, res=True),
    'bf16/BL/8x128': dict(n=28, h=9, w=33, cin=96, cout=136, k=3, bilinear=True),
    'bf16/BL/8x64': dict(n=28, h=9, w=33, cin=96, cout=88, k=3, bilinear=True),
    'bf16/BL/8x32': dict(n=56, h=9, w=33, cin=96, cout=24, k=3, bilinear=True),
    'bf16/BL/8x32+fused': dict(n=2, h=9, w=33, cin=96, cout=24, k=3, bilinear=True, fuse_cout=2, fuse_act='tanh_scaled'),
    'bf16/BL/4x256': dict(n=28, h=5, w=33, cin=96, cout=280, k=3, bilinear=True),
    'bf16/BL/4x128': dict(n=28, h=5, w=33, cin=96, cout=136, k=3, bilinear=True),
    'bf16/BL/4x64': dict(n=2, h=5, w=33, cin=96, cout=88, k=3, bilinear=True),
    'bf16/BL/4x64+res': dict(n=2, h=5, w=33, cin=96, cout=88, k=3, bilinear=True, res=True),
    'bf16/BL/4x32': dict(n=2, h=5, w=33, cin=96, cout=24, k=3, bilinear=True),
    'bf16/BL/4x32+f32': dict(n=2, h=5, w=33, cin=96, cout=24, k=3, bilinear=True, out_f32=True, bn=False, act='none'),
    'bf16/N/16x64': dict(n=112, h=36, w=16, cin=96, cout=88, k=3),
    'bf16/N/8x256': dict(n=56, h=18, w=16, cin=96, cout=280, k=3),
    'bf16/N/8x256+concat_up': dict(n=56, h=18, w=16, cin=96, cout=280, k=3, cin1=64, up1=True),
    'bf16/N/8x256+f32': dict(n=56, h=18, w=16, cin=96, cout=280, k=3, out_f32=True, bn=False, act='tanh_scaled'),
    'bf16/N/8x256+fused': dict(n=2, h=18, w=16, cin=96, cout=250, k=3, fuse_cout=20, fuse_act='none'),
    'bf16/N/8x256+res': dict(n=56, h=18, w=16, cin=96, cout=280, k=3, res=True),
    'bf16/N/8x128': dict(n=56, h=18, w=16, cin=96, cout=136, k=3),
    'bf16/N/8x64': dict(n=56, h=18, w=16, cin=96, cout=88, k=3),
    'bf16/N/8x32': dict(n=112, h=18, w=16, cin=96, cout=24, k=3),
    'bf16/N/8x32+fused': dict(n=2, h=18, w=16, cin=96, cout=24, k=3, fuse_cout=20, fuse_act='none'),
    'bf16/N/4x256': dict(n=56, h=10, w=16, cin=96, cout=280, k=3),
    'bf16/N/4x128': dict(n=56, h=10, w=16, cin=96, cout=136, k=3),
    'bf16/N/4x64': dict(n=2, h=10, w=16, cin=96, cout=88, k=3),
    'bf16/N/4x64+concat_up': dict(n=2, h=10, w=16, cin=96, cout=88, k=3, cin1=64, up1=True),
    'bf16/N/4x64+res': dict(n=2, h=10, w=16, cin=96, cout=88, k=3, res=True),
    'bf16/N/4x32': dict(n=2, h=10, w=16, cin=96, cout=24, k=3),
    'bf16/N/4x32+f32': dict(n=2, h=10, w=16, cin=96, cout=24, k=3, out_f32=True, bn=False, act='tanh_scaled'),
    'e4m3/PW/16x64': dict(n=56, h=17, w=33, cin=192, cout=88, k=1, out_f32=True, bn=False, act='none'),
    'e4m3/PW/8x256': dict(n=28, h=9, w=33, cin=192, cout=280, k=1),
    'e4m3/PW/8x256+f32': dict(n=28, h=9, w=33, cin=192, cout=280, k=1, out_f32=True, bn=False, act='none'),
    'e4m3/PW/8x256+res': dict(n=28, h=9, w=33, cin=192, cout=280, k=1, res=True),
    'e4m3/PW/8x128': dict(n=28, h=9, w=33, cin=192, cout=136, k=1),
    'e4m3/PW/8x64': dict(n=56, h=9, w=33, cin=192, cout=40, k=1),
    'e4m3/PW/8x64+f32': dict(n=28, h=9, w=33, cin=192, cout=88, k=1, out_f32=True, bn=False, act='none'),
    'e4m3/PW/8x32': dict(n=56, h=9, w=33, cin=192, cout=24, k=1, out_f32=True, bn=False, act='none'),
    'e4m3/PW/4x256': dict(n=28, h=5, w=33, cin=192, cout=280, k=1),
    'e4m3/PW/4x128': dict(n=28, h=5, w=33, cin=192, cout=136, k=1),
    'e4m3/PW/4x128+res': dict(n=28, h=5, w=33, cin=192, cout=136, k=1, res=True),
    'e4m3/PW/4x64': dict(n=2, h=5, w=33, cin=192, cout=40, k=1),
    'e4m3/PW/4x64+f32': dict(n=2, h=5, w=33, cin=192, cout=88, k=1, out_f32=True, bn=False, act='none'),
    'e4m3/PW/4x32': dict(n=2, h=5, w=33, cin=192, cout=24, k=1, out_f32=True, bn=False, act='none'),
    'e4m3/S1/16x64': dict(n=56, h=17, w=33, cin=192, cout=88, k=3, out_f32=True, bn=False, act='none'),
    'e4m3/S1/8x256': dict(n=28, h=9, w=33, cin=192, cout=280, k=3),
    'e4m3/S1/8x256+concat_up': dict(n=28, h=9, w=33, cin=192, cout=280, k=3, cin1=128, up1=True),
    'e4m3/S1/8x256+f32': dict(n=28, h=9, w=33, cin=192, cout=280, k=3, out_f32=True, bn=False, act='none'),
    'e4m3/S1/8x256+fused': dict(n=2, h=9, w=33, cin=192, cout=250, k=3, fuse_cout=20, fuse_act='none'),
    'e4m3/S1/8x256+res': dict(n=28, h=9, w=33, cin=192, cout=280, k=3, res=True),
    'e4m3/S1/8x128': dict(n=28, h=9, w=33, cin=192, cout=136, k=3),
    'e4m3/S1/8x64': dict(n=56, h=9, w=33, cin=192, cout=40, k=3),
    'e4m3/S1/8x64+f32': dict(n=28, h=9, w=33, cin=192, cout=88, k=3, out_f32=True, bn=False, act='none'),
    'e4m3/S1/8x32': dict(n=56, h=9, w=33, cin=192, cout=24, k=3, out_f32=True, bn=False, act='none'),
    'e4m3/S1/8x32+fused': dict(n=2, h=9, w=33, cin=192, cout=24, k=3, fuse_cout=20, fuse_act='none'),
    'e4m3/S1/4x256': dict(n=28, h=5, w=33, cin=192, cout=280, k=3),
    'e4m3/S1/4x128': dict(n=28, h=5, w=33, cin=192, cout=136, k=3),
    'e4m3/S1/4x128+concat_up': dict(n=28, h=5, w=33, cin=192, cout=136, k=3, cin1=128, up1=True),
    'e4m3/S1/4x128+res': dict(n=28, h=5, w=33, cin=192, cout=136, k=3, res=True),
    'e4m3/S1/4x64': dict(n=2, h=5, w=33, cin=192, cout=40, k=3),
    'e4m3/S1/4x64+f32': dict(n=2, h=5, w=33, cin=192, cout=88, k=3, out_f32=True, bn=False, act='none'),
    'e4m3/S1/4x32': dict(n=2, h=5, w=33, cin=192, cout=24, k=3, out_f32=True, bn=False, act='none'),
    'e4m3/S2/4x256': dict(n=28, h=9, w=65, cin=192, cout=280, k=3, stride=2),
    'e4m3/S2/4x256+res': dict(n=28, h=9, w=65, cin=192, cout=280, k=3, stride=2, res=True),
    'e4m3/S2/4x128': dict(n=28, h=9, w=65, cin=192, cout=136, k=3, stride=2),
    'e4m3/S2/4x128+res': dict(n=28, h=9, w=65, cin=192, cout=136, k=3, stride=2, res=True),
    'e4m3/S2/4x64': dict(n=2, h=9, w=65, cin=192, cout=40, k=3, stride=2),
    'e4m3/S2/4x64+f32': dict(n=2, h=9, w=65, cin=192, cout=88, k=3, stride=2, out_f32=True, bn=False, act='none'),
    'e4m3/S2/4x32': dict(n=2, h=9, w=65, cin=192, cout=24, k=3, stride=2, out_f32=True, bn=False, act='none'),
    # ---- the three single-tile modes of the bf16 unit.  MODE_S1F (cout_b % 128 == 0 is a condition of the mode): the ragged
    # three-chunk case of S1F_CASES with a real cout of 250; the mode needs 1024 blocks by default, CPN_S1F=2 applies it wherever
    # the kernel fits, as test_conv_two_workgroups_per_cu_mode does
    'bf16/S1F/8x128': dict(n=3, h=44, w=72, cin=96, cout=250, k=3, seed=32),
    'bf16/S1F/8x128+res': dict(n=2, h=20, w=40, cin=96, cout=250, k=3, res=True, seed=33),
    # MODE_S1Q needs 448 tiles of 16 x 32 and cout_b == 64: of S1Q_CASES only the two 4 x 256 x 256 cases run it (whole tiles,
    # cout 64); these are its ragged cases, 2 x 2 tiles per image
    'bf16/S1Q/16x64': dict(n=112, h=17, w=33, cin=96, cout=40, k=5, seed=44),
    'bf16/S1Q/16x64+res': dict(n=112, h=17, w=33, cin=96, cout=40, k=5, res=True, seed=45),
    'bf16/S1Q/16x64+fused': dict(n=112, h=17, w=33, cin=32, cout=40, k=7, fuse_cout=2, fuse_act='tanh_scaled', seed=46),
    # MODE_BR: tests/test_gpu_conv_bridge.py CASES (output 40 x 52: ragged tile rows and columns)
    'bf16/BR/16x64': dict(bridge='bridge_partial_tiles'),
}

ENV = {
    'bf16/S1F/8x128': {'CPN_S1F': '2'},
    'bf16/S1F/8x128+res': {'CPN_S1F': '2'},
}

# edges an entry cannot show: key pattern -> (edges, reason)
EXEMPT = (
    (r'bf16/S2/8x\d+$', ('chunks',), 'MODE_S2 at 8 rows fits the LDS with one halo buffer only: a single 32-channel chunk (9 items, odd)'),
    (r'e4m3/(PW|S1|S2)/[48]x64$', ('cblk',), 'e4m3 NHWC outputs have cout_b % 64 == 0; the +f32 entry of the tile has the partial block'),
    (r'bf16/S1F/', ('cblk',), 'cout_b % 128 == 0 is a condition of MODE_S1F'),
    (r'bf16/S1Q/16x64(\+res)?$', ('cblk',), 'cout_b == 64 == BN is a condition of MODE_S1Q'),
    (r'bf16/S1Q/16x64\+fused$', ('chunks',), 'one chunk of a 7x7: 49 items, padded to 52 (three zero slabs read)'),
    (r'bf16/BR/', ('cblk', 'cpad', 'odd'), 'the bridge kernel runs one shape: 64 -> 64 channels, 3x3 (18 items)'),
)

# instantiations compiled into the library that no valid ConvArgs selects (tests/test_conv_tiles.py drives the query over a
# grid and finds none of them; the argument, with lds_bytes of conv_igemm.hip: halo buffer = ceil(HH * pitch * 4 / 64) KiB,
# pitch 80 for MODE_S2, HH = (TH - 1) * 2 + KH, LDS_MAX = 160 KiB):
UNREACHABLE = {
    'bf16/S2/16x64': 'HH >= 31 (KH >= 1): one halo buffer >= 155 KiB, + 16 KiB of weight slabs + 2.5 KiB column table > 160 KiB',
    'e4m3/S2/16x64': 'as bf16/S2/16x64',
    'e4m3/S2/8x256': 'cin_b % 64 == 0 gives >= 2 chunks of 32, so two halo buffers: HH >= 15, 2 x 75 KiB + >= 8 KiB slabs + 2.5 KiB '
                     '= 160.5 KiB > 160 KiB for every k; choose_tile falls to 4 rows',
    'e4m3/S2/8x128': 'as e4m3/S2/8x256',
    'e4m3/S2/8x64': 'as e4m3/S2/8x256',
    'e4m3/S2/8x32': 'as e4m3/S2/8x256 (8 KiB of slabs is this tile)',
}

# ---- what the existing single-conv cases run (asserted by tests/test_conv_tiles.py, so that a change of the selection rules
# that moves a case to another kernel is seen)
RECORDED_CONV = {
    '1x1_64_64': 'bf16/PW/4x64',
    '1x1_flat_narrow': 'bf16/PW/4x64',
    '1x1_res': 'bf16/PW/4x64',
    '1x1_s2': 'bf16/PW/4x64',
    '3x3_64_64': 'bf16/S1/4x64',
    '3x3_odd_channels': 'bf16/S1/4x32',
    '3x3_256_small_grid_4x64_tile': 'bf16/S1/4x64',
    '3x3_s2': 'bf16/S2/4x64',
    '3x3_grouped_cpg8': 'bf16/S1/4x32',
    '3x3_grouped_cpg64_s2': 'bf16/S2/4x64',
    '3x3_grouped_cpg1': 'bf16/S1/4x32',
    '3x3_concat_up': 'bf16/S1/4x64',
    '3x3_concat_up_pad': 'bf16/S1/4x32',
    '3x3_bridge_up0': 'bf16/S1/4x64',
    '1x1_fpn_lateral': 'bf16/PW/4x64',
    '3x3_c64_th16_tile': 'bf16/S1/16x64',
    '7x7_c64_th16_tile': 'bf16/S1Q/16x64',
    '7x7_head': 'bf16/S1/4x64',
    '7x7_head_256': 'bf16/S1/4x64',
    '7x7_stem_s2': 'bf16/S2/4x64',
    'c64_fused_head_th16': 'bf16/S1Q/16x64',
    'c64_concat_up_partial': 'bf16/S1/4x64',
    'c64_k5_three_chunks': 'bf16/S1/4x64',
    '3x3_256_flagship_tile': 'bf16/S1F/8x128',
    '3x3_256_flagship_concat_up': 'bf16/S1/8x256',
    'fused_head_256_flagship_tile': 'bf16/S1/8x256',
    '3x3_narrow16_flagship': 'bf16/N/4x64',
    '3x3_narrow16_rows24_res': 'bf16/N/4x64',
    '3x3_narrow16_grouped': 'bf16/N/4x32',
    '3x3_narrow16_concat_up': 'bf16/N/4x64',
    '7x7_narrow16_fused_head': 'bf16/N/8x128',
    '5x5_narrow16_f32_out': 'bf16/N/4x32',
    '1x1_flagship_tile': 'bf16/PW/8x256',
    '1x1_flagship_tile_res': 'bf16/PW/8x256',
    'fused_head_256': 'bf16/S1/8x256',
    'fused_head_128_sigmoid': 'bf16/S1/8x128',
    'fused_head_64_tanh_th16': 'bf16/S1Q/16x64',
    'fused_head_64_tanh': 'bf16/S1/8x64',
    'fused_head_small': 'bf16/S1/8x32',
    '7x7_bilinear_src_256': 'bf16/BL/4x64',
    '3x3_bilinear_src_32': 'bf16/BL/4x32',
    'fused_head_64_bilinear': 'bf16/BL/8x64',
    'fused_head_256_bilinear': 'bf16/BL/8x256',
    'final_sigmoid': 'bf16/PW/4x32',
    'final_tanh': 'bf16/PW/4x32',
    'final_fourier': 'bf16/PW/4x32',
}
# (default environment, CPN_S1F=0, CPN_S1F=2): the two switch values test_conv_two_workgroups_per_cu_mode sets
RECORDED_S1F = {
    's1f_3x3_256': ('bf16/S1F/8x128', 'bf16/S1/8x256', 'bf16/S1F/8x128'),
    's1f_3x3_one_chunk': ('bf16/S1/4x64', 'bf16/S1/4x64', 'bf16/S1F/8x128'),
    's1f_3x3_partial_tiles': ('bf16/S1/4x64', 'bf16/S1/4x64', 'bf16/S1F/8x128'),
    's1f_3x3_res': ('bf16/S1/4x64', 'bf16/S1/4x64', 'bf16/S1F/8x128'),
    's1f_5x5_falls_back': ('bf16/S1/4x64', 'bf16/S1/4x64', 'bf16/S1/4x64'),
    's1f_2x2ish_k3_cin2048': ('bf16/S1/4x64', 'bf16/S1/4x64', 'bf16/S1F/8x128'),
    's1f_3x3_512_two_blocks': ('bf16/S1/4x256', 'bf16/S1/4x256', 'bf16/S1F/8x128'),
    's1f_3x3_odd_tile_count': ('bf16/S1/4x64', 'bf16/S1/4x64', 'bf16/S1F/8x128'),
    's1f_3x3_no_bias_none': ('bf16/S1/4x64', 'bf16/S1/4x64', 'bf16/S1F/8x128'),
}
# (default environment, CPN_S1Q=0, CPN_S1Q=1): the two switch values test_conv_four_items_per_step_mode sets
RECORDED_S1Q = {
    's1q_7x7_64_64': ('bf16/S1Q/16x64', 'bf16/S1/16x64', 'bf16/S1Q/16x64'),
    's1q_7x7_fused_head': ('bf16/S1Q/16x64', 'bf16/S1/16x64', 'bf16/S1Q/16x64'),
    's1q_7x7_one_chunk': ('bf16/S1/8x64', 'bf16/S1/8x64', 'bf16/S1/8x64'),
    's1q_5x5_three_chunks_ragged': ('bf16/S1/8x64', 'bf16/S1/8x64', 'bf16/S1/8x64'),
    's1q_7x7_res': ('bf16/S1/8x64', 'bf16/S1/8x64', 'bf16/S1/8x64'),
}
RECORDED_FP8 = {
    '3x3_64_64': 'e4m3/S1/4x64',
    '1x1_128_256': 'e4m3/PW/4x64',
    '1x1_odd_chunks_res': 'e4m3/PW/4x64',
    '3x3_odd_channels': 'e4m3/S1/4x64',
    '3x3_s2': 'e4m3/S2/4x64',
    '7x7_256_small_grid_4x64_tile': 'e4m3/S1/4x64',
    '3x3_concat_up': 'e4m3/S1/4x64',
    '3x3_grouped_cpg8': 'e4m3/S1/4x64',
    '7x7_stem_s2': 'e4m3/S2/4x64',
    'final_f32': 'e4m3/PW/4x32',
    'final_f32_one_block': 'e4m3/PW/4x32',
    'fused_head_64': 'e4m3/S1/8x64',
}
# the three launches of every SUBPIXEL_CASES entry: (HEAD, PHASE, LATERAL)
RECORDED_SUBPIXEL = {
    'sp_64_128_64': ('bf16/S1/4x64', 'bf16/N/4x64', 'bf16/S1/4x64'),
    'sp_padded_channels': ('bf16/S1/4x32', 'bf16/S1/4x32', 'bf16/S1/4x32'),
    'sp_partial_tiles': ('bf16/S1/4x64', 'bf16/S1/4x64', 'bf16/S1/4x64'),
    'sp_flagship_tile': ('bf16/S1/8x256', 'bf16/S1F/8x128', 'bf16/S1F/8x128'),
    'sp_two_cout_blocks': ('bf16/S1/4x256', 'bf16/S1/4x256', 'bf16/S1/4x256'),
    'sp_no_bias': ('bf16/S1/4x32', 'bf16/S1/4x32', 'bf16/S1/4x32'),
    'sp_narrow_lowres': ('bf16/S1/4x128', 'bf16/N/4x128', 'bf16/S1/4x128'),
}


def parse_key(key):
    """'bf16/S1/8x256+res' -> ('bf16', 'S1', 8, 256, 'res')"""
    unit, mode, rest = key.split('/')
    tile, _, variant = rest.partition('+')
    th, bn = tile.split('x')
    return unit, mode, int(th), int(bn), variant


def instantiation(key):
    """The key without its second-epilogue suffix: one compiled kernel."""
    return key.partition('+')[0]


@contextlib.contextmanager
def environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _pad(c, m):
    return (c + m - 1) // m * m


_OPS = {}  # packed one-conv plans by configuration (the shape n, h, w is no part of a plan)


def _ops(kind, cfg):
    import test_gpu_kernels as tk
    from celldetection_amd import graph
    ck = (kind,) + tuple(sorted((k, v) for k, v in cfg.items() if k not in ('n', 'h', 'w')))
    if ck not in _OPS:
        if kind == 'bf16':
            P, sd, _ = tk.conv_plan(**cfg)
            _OPS[ck] = graph.pack(P, sd, 'cpu')[1]
        elif kind == 'e4m3':
            P, sd, _, _ = tk.conv_fp8_plan(cfg)
            _OPS[ck] = graph.pack(P, sd, 'cpu', precision='fp8', act_scales={i: 1. for i in range(len(P.tensors))})[1]
        elif kind == 'subpixel':
            P, sd, _, _ = tk.subpixel_plan(cfg)
            _OPS[ck] = graph.pack(P, sd, 'cpu')[1]
        else:
            import test_gpu_conv_bridge as tb
            P, sd = tb._bridge_plan(cfg['cin'], cfg.get('seed', 0))
            _OPS[ck] = graph.pack(P, sd, 'cpu')[1]
    return _OPS[ck]


def query_conv(cfg):
    """What cpn_conv2d runs for run_conv(**cfg): (mode, TH, BN, WM, WN), from the library, with the strides run_conv passes."""
    from celldetection_amd import _lib
    f32 = cfg.get('out_f32') or cfg.get('fuse_cout')
    return _lib.conv_kernel_info(_ops('bf16', cfg)[0], _lib.PRECISION_BF16, cfg['n'], cfg['h'], cfg['w'], _pad(cfg['cin'], 32),
                                 _pad(cfg.get('cin1', 0), 32), _pad(cfg['cout'], 32) if cfg.get('res') else 0,
                                 0 if f32 else _pad(cfg['cout'], 32))


def query_conv_fp8(cfg):
    """What cpn_conv2d_fp8 runs for run_conv_fp8(**cfg)."""
    from celldetection_amd import _lib
    f32 = cfg.get('out_f32') or cfg.get('fuse_cout')
    return _lib.conv_kernel_info(_ops('e4m3', cfg)[0], _lib.PRECISION_FP8, cfg['n'], cfg['h'], cfg['w'], _pad(cfg['cin'], 64),
                                 _pad(cfg.get('cin1', 0), 64), _pad(cfg['cout'], 64) if cfg.get('res') else 0,
                                 0 if f32 else _pad(cfg['cout'], 64))


def query_bridge(cfg):
    """What cpn_conv_bridge runs for a case of tests/test_gpu_conv_bridge.py."""
    from celldetection_amd import _lib
    return _lib.conv_kernel_info(_ops('bridge', cfg)[2], _lib.PRECISION_BF16, cfg['n'], cfg['h'], cfg['w'], _pad(cfg['cin'], 32),
                                 0, 0, 64)


def query_subpixel(cfg):
    """What the three cpn_conv2d launches of test_subpixel_decoder_conv run: [HEAD, PHASE, LATERAL]."""
    from celldetection_amd import _lib
    ops = _ops('subpixel', cfg)
    n, h, w, c0, c1, cp = cfg['n'], cfg['h'], cfg['w'], _pad(cfg['c0'], 32), _pad(cfg['c1'], 32), _pad(cfg['cout'], 32)
    return [_lib.conv_kernel_info(ops[0], _lib.PRECISION_BF16, n, h, w, c0, c1, 0, cp),
            _lib.conv_kernel_info(ops[1], _lib.PRECISION_BF16, n, h // 2, w // 2, c1, 0, 0, 4 * cp),
            _lib.conv_kernel_info(ops[2], _lib.PRECISION_BF16, n, h, w, c0, 0, 4 * cp, cp)]


def bridge_cfg(name):
    import test_gpu_conv_bridge as tb
    return dict(dict(seed=0), **tb.CASES[name])


def query(key):
    """The library's answer for a TABLE entry under the entry's environment."""
    cfg = TABLE[key]
    with environment(ENV.get(key, {})):
        if 'bridge' in cfg:
            return query_bridge(bridge_cfg(cfg['bridge']))
        return (query_conv_fp8 if key.startswith('e4m3/') else query_conv)(cfg)


def info_key(unit, info):
    return f'{unit}/{info[0]}/{info[1]}x{info[2]}'


def out_size(cfg):
    if 'bridge' in cfg:
        c = bridge_cfg(cfg['bridge'])
        return 2 * c['h'], 2 * c['w']
    k, s = cfg['k'], cfg.get('stride', 1)
    return (cfg['h'] + 2 * (k // 2) - k) // s + 1, (cfg['w'] + 2 * (k // 2) - k) // s + 1


def edges(key, info):
    """{edge: shown} of a TABLE entry on the tile the library returned for it."""
    unit, cfg = parse_key(key)[0], TABLE[key]
    mode, th, bn = info[:3]
    ho, wo = out_size(cfg)
    hv = ho // 2 if mode == 'N' else ho
    if 'bridge' in cfg:
        c = bridge_cfg(cfg['bridge'])
        n, cout, cout_b, chunks, taps, fused = c['n'], 64, 64, 2, 9, False
    else:
        kc = 64 if unit == 'e4m3' else 32
        nhwc = not (cfg.get('out_f32') or cfg.get('fuse_cout'))
        n, cout, fused = cfg['n'], cfg['cout'], bool(cfg.get('fuse_cout'))
        cout_b = _pad(cout, kc if nhwc else 32)
        chunks = (_pad(cfg['cin'], kc) + (_pad(cfg['cin1'], kc) if cfg.get('cin1') else 0)) // kc
        taps = cfg['k'] ** 2
    return dict(n2=n >= 2, row=hv % th != 0, col=mode == 'N' or wo % 32 != 0, full=hv >= th and (mode == 'N' or wo >= 32),
                cblk=bn == 32 or fused or cout_b % bn != 0, cpad=cout % 32 != 0, chunks=chunks >= 2, odd=chunks * taps % 2 == 1)


def exempt(key):
    out = set()
    for pattern, names, _ in EXEMPT:
        if re.match(pattern, key):
            out.update(names)
    return out


# ---- the instantiations a built library holds, from its dynamic symbol table (names only)
_SYMBOL = re.compile(r'^_ZN(3cpn|7cpn_fp8)17conv_igemm_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEEvN\w*8ConvArgsE$')


def dynamic_symbols(path):
    """Names in .dynsym of an ELF64 little-endian shared object."""
    with open(path, 'rb') as f:
        data = f.read()
    assert data[:6] == b'\x7fELF\x02\x01', 'not an ELF64 little-endian file'
    shoff, = struct.unpack_from('<Q', data, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', data, 0x3a)
    sections = [struct.unpack_from('<IIQQQQIIQQ', data, shoff + i * shentsize) for i in range(shnum)]
    names = []
    for sec in sections:
        if sec[1] != 11:  # SHT_DYNSYM
            continue
        off, size, link, entsize = sec[4], sec[5], sec[6], sec[9]
        stroff = sections[link][4]
        for i in range(size // entsize):
            st_name, = struct.unpack_from('<I', data, off + i * entsize)
            end = data.index(b'\0', stroff + st_name)
            names.append(data[stroff + st_name:end].decode())
    return names


def library_instantiations(path=None):
    """{'bf16/S1/8x256': (WM, WN), ...}: every conv_igemm_kernel<TH, BN, WM, WN, MODE> kernel handle the library exports."""
    from celldetection_amd import _lib
    out = {}
    for name in dynamic_symbols(path or _lib.LIB_PATH):
        m = _SYMBOL.match(name)
        if m:
            th, bn, wm, wn, mode = (int(x) for x in m.groups()[1:])
            out[f'{"bf16" if m.group(1) == "3cpn" else "e4m3"}/{_lib.CONV_MODE_NAMES[mode]}/{th}x{bn}'] = (wm, wn)
    return out


def locate(key, info, index, shape):
    """Where a failing output element (index into the NCHW result of `shape`) lies in the tiling the library named."""
    mode, th, bn = info[:3]
    _, c, y, x = index
    _, _, ho, wo = shape
    if mode == 'N':  # tiles of 2 TH rows x 16 columns
        th, x, wo = 2 * th, 0, 32
    cfg = TABLE[key]
    where = []
    if ho % th and y >= ho - ho % th:
        where.append('edge row tile')
    if wo % 32 and x >= wo - wo % 32:
        where.append('edge column tile')
    cout = shape[1]
    if not cfg.get('fuse_cout') and cout > bn and c >= (cout - 1) // bn * bn:
        where.append('last channel block')
    return f'{key} <{info[1]},{info[2]},{info[3]},{info[4]}> {mode}: worst element {tuple(index)} in ' + \
           (', '.join(where) if where else 'an interior tile')


def worst(got, lo, hi, ref):
    """Index and |got - ref| / bound of the worst element (the measure of conv_bounds.check)."""
    import torch
    got, ref = got.double(), ref.double().expand_as(got)
    side = torch.where(got >= ref, hi - ref, ref - lo).clamp_min(0.)
    dev = (got - ref).abs()
    ratio = torch.where(dev == 0, torch.zeros_like(dev), dev / side)
    ratio = torch.nan_to_num(torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float('inf'))), nan=float('inf'))
    i = int(torch.argmax(ratio))
    return tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape)), float(ratio.reshape(-1)[i])
