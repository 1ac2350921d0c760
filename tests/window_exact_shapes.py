"""Shapes of tests/test_gpu_window_exact.py: the smallest at which the window kernels can still go wrong.  Kept apart from the GPU
suite so that tests/test_host_window_kernel_model.py can check, without a device, that they have the properties the suite relies on."""
from pytorch_connectomics_amd import _native as nat

# window, the swaps it is legal for: every window has more than 256 voxels (two workgroups) and no multiple of 256 (ragged last one)
WINDOWS = (((5, 7, 9), ()),
           ((5, 8, 8), (nat.VIEW_SWAP_YX,)),
           ((9, 9, 5), (nat.VIEW_SWAP_ZY,)),
           ((9, 5, 9), (nat.VIEW_SWAP_ZX,)),
           ((7, 7, 7), (nat.VIEW_SWAP_YX, nat.VIEW_SWAP_ZY, nat.VIEW_SWAP_ZX)))


def volume_of(roi):
    """a little more than two windows per axis, odd: (5, 7, 9) -> (11, 15, 19)"""
    return tuple(2 * int(r) + 1 for r in roi)


def blend_starts(roi):
    """Window positions of the blend tests, in the order they are added: four windows that share voxels in the middle of the volume,
    one overhanging the three low faces (negative starts) and one the three high faces; some voxels stay uncovered."""
    h = [int(r) // 2 for r in roi]
    return [(h[0], h[1], h[2]),
            (int(roi[0]) + 3, int(roi[1]) + 2, int(roi[2]) + 4),
            (h[0] + 1, h[1], h[2] + 1),
            (-2, -1, -3),
            (h[0], h[1] + 2, h[2]),
            (h[0] - 1, h[1] + 1, h[2] + 1)]


STRIDE_N = 8192 * 256 + 3                       # one element more than the 8192-block cap of the flat kernels covers in one trip
FLAT_SIZES = (1, 255, 257, STRIDE_N)
CAST_SIZES = (1, 2, 3, 5, 1022, 1023, 8192 * 1024 + 1)     # scale_cast: four elements per thread, scalar tail, 8192-block cap
NORM_N = 2 * 8192 + 37                          # window_normalize: three statistics slots, the last one ragged
# channels-last activation, (voxels, C): the flat float4 kernel (65536 blocks of 256 threads, four elements each) takes a second trip
# from 65536 * 256 * 4 + 4 * C elements on; the smallest number of whole 7-channel voxels there whose elements are whole float4s
ACT_FLAT = (9586988, 7)
ACT_RAGGED = (1001, 7)                          # (voxels, C) with voxels * C % 4 != 0: the per-voxel form
RESAMPLE_SECOND = (7, 9, 5)                     # a second region: 315 voxels, two workgroups
