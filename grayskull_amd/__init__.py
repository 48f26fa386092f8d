"""grayskull_amd -- MI355X-native implementation of Grayskull's pixel-array hot path.

Python mirror of the C boundary (include/grayskull.h + include/grayskull_hip.h) over ctypes.
Names, argument order and error behaviour follow the reference header
(/root/reference/grayskull.h; each wrapper cites the definition it fronts).  All compute
happens in libgrayskull_hip.so (hand-written HIP kernels, gfx950); there is no Python or CPU
fallback -- if the library is missing this module raises at first use.

Image arguments may be numpy uint8 arrays (host memory: staged through the GPU, synchronous)
or torch CUDA tensors / anything with ``data_ptr()`` (device memory: zero-copy).

    import grayskull_amd as gs
    gs.blur(dst, src, 2); gs.sobel(edges, dst); t = gs.otsu_threshold(edges); gs.threshold(edges, t)
"""
import ctypes as C
import os

import numpy as np

from ._abi import (BLOB_DTYPE, CONTOUR_DTYPE, GsImage, GsLbpCascade, GsPoint, GsRect, KEYPOINT_DTYPE, MATCH_DTYPE, POINT_DTYPE,
                   RECT_DTYPE)
from .cascade import Cascade

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIBRARY = os.path.join(_HERE, "libgrayskull_hip.so")

__all__ = ["Grayskull", "Cascade", "lib", "BLOB_DTYPE", "CONTOUR_DTYPE", "KEYPOINT_DTYPE", "MATCH_DTYPE", "POINT_DTYPE", "RECT_DTYPE"]


def _ptr(a):
    """address of a numpy array or of a torch tensor (host or device)"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        if not a.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return a.data_ptr()
    if isinstance(a, int):
        return a
    raise TypeError("expected numpy array, torch tensor or raw address, got %r" % type(a))


def _img(a):
    if a.ndim != 2:
        raise ValueError("expected a 2-D (h, w) uint8 image")
    return GsImage(int(a.shape[1]), int(a.shape[0]), _ptr(a))


_SIGS = {
    # drop-in (include/grayskull.h)
    "gs_blur": (None, [GsImage, GsImage, C.c_uint]),
    "gs_sobel": (None, [GsImage, GsImage]),
    "gs_erode": (None, [GsImage, GsImage]),
    "gs_dilate": (None, [GsImage, GsImage]),
    "gs_histogram": (None, [GsImage, C.c_void_p]),
    "gs_otsu_threshold": (C.c_uint8, [GsImage]),
    "gs_threshold": (None, [GsImage, C.c_uint8]),
    "gs_integral": (None, [GsImage, C.c_void_p]),
    "gs_lbp_window": (C.c_uint, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_int, C.c_int,
                                 C.c_float]),
    "gs_lbp_detect": (C.c_uint, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_uint,
                                 C.c_float, C.c_float, C.c_float, C.c_int]),
    "gs_fast": (C.c_uint, [GsImage, GsImage, C.c_void_p, C.c_uint, C.c_uint]),
    "gs_compute_orientation": (C.c_float, [GsImage, C.c_uint, C.c_uint, C.c_uint]),
    "gs_brief_descriptor": (None, [GsImage, C.c_void_p]),
    "gs_orb_extract": (C.c_uint, [GsImage, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p]),
    "gs_match_orb": (C.c_uint, [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint,
                                C.c_float]),
    # the reference's GS_NO_STDLIB trig flavour (ref :68-88): what include/grayskull.h binds under that macro
    "gs_compute_orientation_nostdlib": (C.c_float, [GsImage, C.c_uint, C.c_uint, C.c_uint]),
    "gs_brief_descriptor_nostdlib": (None, [GsImage, C.c_void_p]),
    "gs_orb_extract_nostdlib": (C.c_uint, [GsImage, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p]),
    "gs_adaptive_threshold": (None, [GsImage, GsImage, C.c_uint, C.c_int]),
    "gs_filter": (None, [GsImage, GsImage, GsImage, C.c_uint]),
    "gs_downsample": (None, [GsImage, GsImage]),
    "gs_crop": (None, [GsImage, GsImage, GsRect]),
    "gs_copy": (None, [GsImage, GsImage]),
    "gs_resize_nn": (None, [GsImage, GsImage]),
    "gs_resize": (None, [GsImage, GsImage]),
    "gs_match_template": (None, [GsImage, GsImage, GsImage]),
    "gs_find_best_match": (GsPoint, [GsImage]),
    "gs_blobs": (C.c_uint, [GsImage, C.c_void_p, C.c_void_p, C.c_uint]),
    "gs_blob_corners": (None, [GsImage, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gs_trace_contour": (None, [GsImage, GsImage, C.c_void_p]),
    "gs_perspective_correct": (None, [GsImage, GsImage, C.c_void_p]),
    # runtime + batch (include/grayskull_hip.h)
    "gsh_version": (C.c_char_p, []),
    "gsh_device_count": (C.c_int, []),
    "gsh_set_device": (None, [C.c_int]),
    "gsh_set_stream": (None, [C.c_void_p]),
    "gsh_get_stream": (C.c_void_p, []),
    "gsh_set_async": (None, [C.c_int]),
    "gsh_sync": (None, []),
    "gsh_tune": (None, [C.c_int, C.c_int]),
    "gsh_profile": (None, [C.c_int]),
    "gsh_profile_read": (C.c_uint, [C.POINTER(C.c_double)]),
    "gsh_fast_score_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint]),
    "gsh_shutdown": (None, []),
    "gsh_malloc": (C.c_void_p, [C.c_size_t]),
    "gsh_free": (None, [C.c_void_p]),
    "gsh_host_alloc": (C.c_void_p, [C.c_size_t]),
    "gsh_host_free": (None, [C.c_void_p]),
    "gsh_memset": (None, [C.c_void_p, C.c_int, C.c_size_t]),
    "gsh_upload": (None, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "gsh_download": (None, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "gsh_is_device_ptr": (C.c_int, [C.c_void_p]),
    "gsh_blur_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint]),
    "gsh_sobel_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint]),
    "gsh_erode_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint]),
    "gsh_dilate_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint]),
    "gsh_morph_batch": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_uint]),
    "gsh_histogram_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]),
    "gsh_otsu_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]),
    "gsh_threshold_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint8]),
    "gsh_threshold_batch_dev": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]),
    "gsh_blur_sobel_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint]),
    "gsh_edge_pipeline_batch": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint,
                                       C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]),
    "gsh_integral_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]),
    "gsh_cascade_create": (C.c_void_p, [C.c_void_p]),
    "gsh_cascade_destroy": (None, [C.c_void_p]),
    "gsh_lbp_detect_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint,
                                    C.c_void_p, C.c_void_p, C.c_uint, C.c_float, C.c_float,
                                    C.c_float, C.c_int]),
    "gsh_lbp_count_evaluated": (None, [C.c_void_p]),
    "gsh_lbp_window_count": (C.c_uint64, [C.c_void_p, C.c_uint, C.c_uint, C.c_float, C.c_float,
                                          C.c_float, C.c_int]),
    "gsh_fast_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p,
                              C.c_void_p, C.c_uint, C.c_uint]),
    "gsh_orb_extract": (C.c_uint, [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p,
                                   C.c_uint, C.c_uint]),
    "gsh_orb_extract_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_uint, C.c_uint]),
    "gsh_orb_extract_batch_nostdlib": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_uint, C.c_uint]),
    "gsh_orb_pyramid_buffer_bytes": (C.c_size_t, [C.c_uint, C.c_uint, C.c_uint]),
    "gsh_orb_extract_pyramid": (C.c_uint, [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p,
                                           C.c_uint, C.c_uint, C.c_uint]),
    "gsh_pyramid_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint]),
    "gsh_orb_pyramid_batch_buffer_bytes": (C.c_size_t, [C.c_uint, C.c_uint, C.c_uint, C.c_uint]),
    "gsh_orb_extract_pyramid_batch_nostdlib": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint]),
    "gsh_orb_extract_pyramid_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint]),
    "gsh_orb_pyramid_batch_times": (None, [C.POINTER(C.c_double)]),
    "gsh_orb_pyramid_buffer_fill_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint]),
    "gsh_match_orb_dev": (None, [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_void_p,
                                 C.c_void_p, C.c_uint, C.c_float]),
    "gsh_match_orb_batch": (None, [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_void_p, C.c_uint,
                                   C.c_uint, C.c_void_p, C.c_void_p, C.c_uint, C.c_float]),
    "gsh_adaptive_threshold_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint,
                                            C.c_uint, C.c_int]),
    "gsh_filter_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p,
                                C.c_uint, C.c_uint, C.c_uint]),
    "gsh_downsample_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint]),
    "gsh_crop_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, GsRect]),
    "gsh_resize_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_uint]),
    "gsh_resize_nn_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_uint]),
    "gsh_crop_resize_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p,
                                      C.c_void_p, C.c_uint, C.c_int]),
    "gsh_match_template_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_uint,
                                         C.c_void_p]),
    "gsh_find_best_match_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]),
    "gsh_locate_template_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_uint,
                                          C.c_void_p, C.c_void_p]),
    "gsh_match_templates_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_uint,
                                         C.c_void_p]),
    "gsh_locate_templates_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_uint,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsh_locate_template_windows_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_uint,
                                                  C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]),
    "gsh_match_template_windows_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint, C.c_uint,
                                                 C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]),
    "gsh_search_windows_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p]),
    "gsh_blobs_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_uint]),
    "gsh_blob_corners_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p,
                                       C.c_void_p]),
    "gsh_perspective_correct_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_uint, C.c_uint,
                                              C.c_uint, C.c_void_p]),
    "gsh_blob_largest_batch": (None, [C.c_void_p, C.c_uint, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]),
    "gsh_blob_paint_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_uint,
                                    C.c_void_p]),
    "gsh_threshold_batch_dev_offset": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_int]),
    "gsh_trace_contours_batch": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_uint,
                                         C.c_void_p, C.c_void_p]),
    "gsh_blob_contour_starts_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_uint,
                                              C.c_void_p, C.c_void_p]),
    "gsh_synth_batch": (None, [C.c_void_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint32]),
    "gsh_checksum_batch": (None, [C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p]),
    # multi-GPU control plane of one-process host programs (csrc/gs_comm.cpp; RCCL looked up at run time)
    "gsh_comm_init_all": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int)]),
    "gsh_comm_destroy_all": (None, [C.POINTER(C.c_void_p), C.c_int]),
    "gsh_comm_rank": (C.c_int, [C.c_void_p]),
    "gsh_comm_world": (C.c_int, [C.c_void_p]),
    "gsh_comm_backend": (C.c_char_p, [C.c_void_p]),
    "gsh_comm_broadcast": (None, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "gsh_comm_all_gather": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "gsh_comm_all_reduce_u64": (None, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "gsh_comm_all_reduce_f64": (None, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
}
EXPORTED_SYMBOLS = tuple(sorted(_SIGS))
# -DGS_EXPERIMENT builds only (build_variants/libgs_experiment.so): bound when the library has them
_EXPERIMENT_SIGS = {
    "gsh_probe_strip_copy": (None, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_uint]),
}


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so / libhsa-runtime64.so and load them by file
    name; libgrayskull_hip.so needs `libamdhip64.so.7` by SONAME.  If this library comes first, the
    system runtime is loaded, `import torch` later loads a SECOND runtime and finds no GPU
    ("No HIP GPUs are available").  So when torch is installed but not imported yet, load its
    runtime first: ours then binds to it by SONAME and a later `import torch` finds it loaded.
    Without torch nothing happens and the system ROCm runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if not spec or not spec.origin:
        return
    libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        f = os.path.join(libdir, name)
        if os.path.exists(f):
            try:
                C.CDLL(f, mode=C.RTLD_GLOBAL)
            except OSError:
                return


class Grayskull:
    """Bound libgrayskull_hip.so.  `path` is for the test-suite's emulator build only."""

    def __init__(self, path=None):
        path = path or HIP_LIBRARY
        if not os.path.exists(path):
            raise ImportError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). grayskull_amd has no CPU fallback." % path)
        self.path = path
        if os.path.abspath(path) == os.path.abspath(HIP_LIBRARY):
            _share_torch_hip_runtime()
        self.c = C.CDLL(path)
        for name, (res, args) in _SIGS.items():
            f = getattr(self.c, name)
            f.restype, f.argtypes = res, args
        for name, (res, args) in _EXPERIMENT_SIGS.items():
            if hasattr(self.c, name):
                f = getattr(self.c, name)
                f.restype, f.argtypes = res, args

    # ------------------------------------------------------------------ runtime
    def version(self):
        return self.c.gsh_version().decode()

    def device_count(self):
        return int(self.c.gsh_device_count())

    def set_device(self, i):
        self.c.gsh_set_device(int(i))

    def use_torch_stream(self):
        """enqueue on torch's current stream (so torch.cuda.Event brackets see the kernels)"""
        import torch
        self.c.gsh_set_stream(C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def set_stream(self, handle):
        self.c.gsh_set_stream(C.c_void_p(handle))

    def set_async(self, on):
        self.c.gsh_set_async(1 if on else 0)

    def shutdown(self):
        """gsh_shutdown: release the calling thread's device scratch, streams and events"""
        self.c.gsh_shutdown()

    def sync(self):
        self.c.gsh_sync()

    def tune(self, key, value):
        self.c.gsh_tune(int(key), int(value))

    def profile(self, on):
        """True / False, or an int > 1 = switch on and pre-create that many event pairs"""
        self.c.gsh_profile(int(on))

    def profile_read(self):
        """(launches bracketed since the last read, their summed duration in ms)"""
        ms = C.c_double(0.0)
        n = self.c.gsh_profile_read(C.byref(ms))
        return int(n), float(ms.value)

    def fast_score_batch(self, score, img, threshold):
        """pass 1 of gs_fast alone: the score map of n frames"""
        n, h, w = self._nhw(img)
        self.c.gsh_fast_score_batch(_ptr(score), _ptr(img), w, h, n, threshold)

    probe_fast_score = fast_score_batch  # the name the measurement scripts of rounds 2-4 use

    @property
    def experiment(self):
        """whether this is a -DGS_EXPERIMENT build (probes and result-changing tune keys available)"""
        return hasattr(self.c, "gsh_probe_strip_copy")

    def probe_strip_copy(self, dst, src):
        """experiment builds only (UB_LIB=build_variants/libgs_experiment.so)"""
        n, h, w = self._nhw(src)
        self.c.gsh_probe_strip_copy(_ptr(dst), _ptr(src), w, h, n)

    # ------------------------------------------------------------------ drop-in (one image)
    def blur(self, dst, src, radius):  # grayskull.h:268
        self.c.gs_blur(_img(dst), _img(src), radius)

    def sobel(self, dst, src):  # grayskull.h:306
        self.c.gs_sobel(_img(dst), _img(src))

    def erode(self, dst, src):  # grayskull.h:303
        self.c.gs_erode(_img(dst), _img(src))

    def dilate(self, dst, src):  # grayskull.h:304
        self.c.gs_dilate(_img(dst), _img(src))

    def histogram(self, img):  # grayskull.h:199
        hist = np.zeros(256, np.uint32)
        self.c.gs_histogram(_img(img), hist.ctypes.data)
        return hist

    def otsu_threshold(self, img):  # grayskull.h:205
        return int(self.c.gs_otsu_threshold(_img(img)))

    def threshold(self, img, t):  # grayskull.h:225 (in place)
        self.c.gs_threshold(_img(img), t)

    def adaptive_threshold(self, dst, src, radius, c):  # grayskull.h:230
        self.c.gs_adaptive_threshold(_img(dst), _img(src), radius, c)

    def filter(self, dst, src, kernel, norm):  # grayskull.h:255; kernel: int8-valued 2-D array
        k = np.ascontiguousarray(kernel).astype(np.int8).view(np.uint8)
        self.c.gs_filter(_img(dst), _img(src), _img(k), norm)

    def downsample(self, dst, src):  # grayskull.h:189
        self.c.gs_downsample(_img(dst), _img(src))

    def crop(self, dst, src, x, y, w, h):  # grayskull.h:154
        self.c.gs_crop(_img(dst), _img(src), GsRect(x, y, w, h))

    def copy(self, dst, src):  # grayskull.h:160
        self.c.gs_copy(_img(dst), _img(src))

    def resize(self, dst, src, nearest=False):  # grayskull.h:171 / :164
        (self.c.gs_resize_nn if nearest else self.c.gs_resize)(_img(dst), _img(src))

    def match_template(self, img, tmpl, result):  # grayskull.h:705
        self.c.gs_match_template(_img(img), _img(tmpl), _img(result))

    def find_best_match(self, result):  # grayskull.h:726
        p = self.c.gs_find_best_match(_img(result))
        return int(p.x), int(p.y)

    def blobs(self, img, nblobs, labels=None):
        """grayskull.h:330 -> (BLOB_DTYPE records of the m blobs, labels).  `labels` (h, w) uint16 may be a device
        tensor (zero-copy); by default a host array is allocated and returned."""
        if labels is None:
            labels = np.zeros(img.shape, np.uint16)
        recs = np.zeros(max(nblobs, 1), BLOB_DTYPE)
        m = self.c.gs_blobs(_img(img), _ptr(labels), recs.ctypes.data, nblobs)
        return recs[:m].copy(), labels

    def blob_corners(self, img, labels, blob):
        """grayskull.h:404: blob is one BLOB_DTYPE record -> [(x, y)] * 4 in the order tl, tr, br, bl"""
        b = np.ascontiguousarray(np.asarray(blob, BLOB_DTYPE).reshape(1))
        c = np.zeros(4, POINT_DTYPE)
        self.c.gs_blob_corners(_img(img), _ptr(labels), b.ctypes.data, c.ctypes.data)
        return [(int(p["x"]), int(p["y"])) for p in c]

    def perspective_correct(self, dst, src, corners):
        """grayskull.h:423: corners = 4 (x, y) pairs tl, tr, br, bl"""
        c = np.ascontiguousarray(np.asarray(corners, np.uint32).reshape(4, 2))
        self.c.gs_perspective_correct(_img(dst), _img(src), c.ctypes.data)

    def trace_contour(self, img, visited, start):
        """grayskull.h:446: the walk from start = (x, y) -> one CONTOUR_DTYPE record (box, start, length); `visited`
        (h, w) uint8, host or device, is marked in place.  Where the reference's walk would never end, the values it
        converges to."""
        c = np.zeros(1, CONTOUR_DTYPE)
        c["sx"], c["sy"] = int(start[0]) & 0xFFFFFFFF, int(start[1]) & 0xFFFFFFFF
        self.c.gs_trace_contour(_img(img), _img(visited), c.ctypes.data)
        return c[0]

    def integral(self, src, ii=None):  # grayskull.h:744
        if ii is None:
            ii = np.zeros(src.shape, np.uint32)
        self.c.gs_integral(_img(src), _ptr(ii))
        return ii

    def lbp_window(self, cascade, ii, x, y, scale):  # grayskull.h:790
        ih, iw = ii.shape
        return int(self.c.gs_lbp_window(C.addressof(cascade.as_struct()), _ptr(ii), iw, ih, x, y,
                                        scale))

    def lbp_detect(self, cascade, ii, max_rects, scale_factor, min_scale, max_scale, step):
        """grayskull.h:815 -> RECT_DTYPE array of the detections, reference order"""
        ih, iw = ii.shape
        rects = np.zeros(max(max_rects, 1), RECT_DTYPE)
        n = self.c.gs_lbp_detect(C.addressof(cascade.as_struct()), _ptr(ii), iw, ih,
                                 rects.ctypes.data, max_rects, scale_factor, min_scale, max_scale,
                                 step)
        return rects[:n].copy()

    def fast(self, img, scoremap, nkps, threshold):  # grayskull.h:482
        kps = np.zeros(max(nkps, 1), KEYPOINT_DTYPE)
        n = self.c.gs_fast(_img(img), _img(scoremap), kps.ctypes.data, nkps, threshold)
        return kps[:n].copy()

    def compute_orientation(self, img, x, y, r=15):  # grayskull.h:608
        return float(self.c.gs_compute_orientation(_img(img), x, y, r))

    def brief_descriptor(self, img, x, y, angle):  # grayskull.h:623
        kp = np.zeros(1, KEYPOINT_DTYPE)
        kp["x"], kp["y"], kp["angle"] = x, y, angle
        self.c.gs_brief_descriptor(_img(img), kp.ctypes.data)
        return kp["desc"][0].copy()

    def orb_extract(self, img, nkps, threshold, scoremap):  # grayskull.h:651
        kps = np.zeros(max(nkps, 1), KEYPOINT_DTYPE)
        n = self.c.gs_orb_extract(_img(img), kps.ctypes.data, nkps, threshold, _ptr(scoremap))
        return kps[:n].copy()

    # the same three under -DGS_NO_STDLIB (include/grayskull.h binds them to these symbols; ref :68-88)
    def compute_orientation_nostdlib(self, img, x, y, r=15):
        return float(self.c.gs_compute_orientation_nostdlib(_img(img), x, y, r))

    def brief_descriptor_nostdlib(self, img, x, y, angle):
        kp = np.zeros(1, KEYPOINT_DTYPE)
        kp["x"], kp["y"], kp["angle"] = x, y, angle
        self.c.gs_brief_descriptor_nostdlib(_img(img), kp.ctypes.data)
        return kp["desc"][0].copy()

    def orb_extract_nostdlib(self, img, nkps, threshold, scoremap):
        kps = np.zeros(max(nkps, 1), KEYPOINT_DTYPE)
        n = self.c.gs_orb_extract_nostdlib(_img(img), kps.ctypes.data, nkps, threshold, _ptr(scoremap))
        return kps[:n].copy()

    def match_orb(self, k1, k2, max_matches, max_distance):  # grayskull.h:680
        k1 = np.ascontiguousarray(k1, KEYPOINT_DTYPE)
        k2 = np.ascontiguousarray(k2, KEYPOINT_DTYPE)
        out = np.zeros(max(max_matches, 1), MATCH_DTYPE)
        n = self.c.gs_match_orb(k1.ctypes.data, len(k1), k2.ctypes.data, len(k2), out.ctypes.data,
                                max_matches, max_distance)
        return out[:n].copy()

    # ------------------------------------------------------------------ batches (device resident)
    @staticmethod
    def _nhw(a):
        if a.ndim != 3:
            raise ValueError("expected (n, h, w)")
        return int(a.shape[0]), int(a.shape[1]), int(a.shape[2])

    def blur_batch(self, dst, src, radius):
        n, h, w = self._nhw(src)
        self.c.gsh_blur_batch(_ptr(dst), _ptr(src), w, h, n, radius)

    def sobel_batch(self, dst, src):
        n, h, w = self._nhw(src)
        self.c.gsh_sobel_batch(_ptr(dst), _ptr(src), w, h, n)

    def erode_batch(self, dst, src):
        n, h, w = self._nhw(src)
        self.c.gsh_erode_batch(_ptr(dst), _ptr(src), w, h, n)

    def dilate_batch(self, dst, src):
        n, h, w = self._nhw(src)
        self.c.gsh_dilate_batch(_ptr(dst), _ptr(src), w, h, n)

    def morph_batch(self, dst, src, iterations, dilate, tmp=None):
        """gsh_morph_batch: `iterations` applications of gs_erode (dilate false) / gs_dilate to src (n, h, w) uint8 in
        ceil(iterations / 4) passes; tmp (n, h, w) uint8 or None = the library's scratch, used beyond 4 iterations"""
        n, h, w = self._nhw(src)
        self.c.gsh_morph_batch(_ptr(dst), _ptr(src), _ptr(tmp), w, h, n, 1 if dilate else 0, int(iterations))

    def histogram_batch(self, img, hist):
        n, h, w = self._nhw(img)
        self.c.gsh_histogram_batch(_ptr(img), w, h, n, _ptr(hist))

    def otsu_batch(self, img, hist_scratch, thr):
        n, h, w = self._nhw(img)
        self.c.gsh_otsu_batch(_ptr(img), w, h, n, _ptr(hist_scratch), _ptr(thr))

    def threshold_batch(self, img, t):
        n, h, w = self._nhw(img)
        if isinstance(t, int):
            self.c.gsh_threshold_batch(_ptr(img), w, h, n, t)
        else:
            self.c.gsh_threshold_batch_dev(_ptr(img), w, h, n, _ptr(t))

    def blur_sobel_batch(self, dst, src, radius):
        n, h, w = self._nhw(src)
        self.c.gsh_blur_sobel_batch(_ptr(dst), _ptr(src), w, h, n, radius)

    def edge_pipeline_batch(self, dst, tmp, src, radius, hist_scratch, thr):
        n, h, w = self._nhw(src)
        self.c.gsh_edge_pipeline_batch(_ptr(dst), _ptr(tmp) if tmp is not None else None, _ptr(src), w, h, n, radius,
                                       _ptr(hist_scratch), _ptr(thr))

    def integral_batch(self, src, ii):
        n, h, w = self._nhw(src)
        self.c.gsh_integral_batch(_ptr(src), w, h, n, _ptr(ii))

    def cascade_create(self, cascade):
        return DeviceCascade(self, cascade)

    def lbp_detect_batch(self, dcascade, ii, rects, counts, max_rects, scale_factor, min_scale,
                         max_scale, step):
        n, h, w = self._nhw(ii)
        self.c.gsh_lbp_detect_batch(dcascade.handle, _ptr(ii), w, h, n, _ptr(rects), _ptr(counts),
                                    max_rects, scale_factor, min_scale, max_scale, step)

    def lbp_count_evaluated(self, counter):
        """counter: FOUR-element int64 device tensor (zeroed by the caller): [windows of chunks that were not
        skipped, weak classifiers evaluated, dword table loads issued, windows through the prefilter]; None
        switches the counting kernels off"""
        self.c.gsh_lbp_count_evaluated(_ptr(counter) if counter is not None else None)

    def lbp_window_count(self, cascade, iw, ih, scale_factor, min_scale, max_scale, step):
        return int(self.c.gsh_lbp_window_count(C.addressof(cascade.as_struct()), iw, ih,
                                               scale_factor, min_scale, max_scale, step))

    def fast_batch(self, img, scoremap, kps, counts, nkps, threshold):
        n, h, w = self._nhw(img)
        self.c.gsh_fast_batch(_ptr(img), _ptr(scoremap), w, h, n, _ptr(kps), _ptr(counts), nkps,
                              threshold)

    def orb_extract_dev(self, img, scoremap, nkps, threshold):
        h, w = int(img.shape[0]), int(img.shape[1])
        kps = np.zeros(max(nkps, 1), KEYPOINT_DTYPE)
        n = self.c.gsh_orb_extract(_ptr(img), w, h, _ptr(scoremap), kps.ctypes.data, nkps, threshold)
        return kps[:n].copy()

    def orb_extract_batch_dev(self, imgs, scoremaps, nkps, threshold):
        """n same-size device frames -> list of per-frame keypoint arrays (two host round trips in total)"""
        n, h, w = self._nhw(imgs)
        kps = np.zeros((n, max(nkps, 1)), KEYPOINT_DTYPE)
        counts = np.zeros(n, np.uint32)
        self.c.gsh_orb_extract_batch(_ptr(imgs), w, h, n, _ptr(scoremaps), kps.ctypes.data, counts.ctypes.data, nkps,
                                     threshold)
        return [kps[f, :int(counts[f])].copy() for f in range(n)]

    def orb_pyramid_buffer_bytes(self, w, h, n_levels):
        return int(self.c.gsh_orb_pyramid_buffer_bytes(w, h, n_levels))

    def orb_extract_batch_nostdlib(self, imgs, scoremaps, kps, counts, nkps, threshold):
        """device-resident gs_orb_extract (GS_NO_STDLIB trig): kps (n, nkps, 12) int32 and counts (n) device tensors"""
        n, h, w = self._nhw(imgs)
        self.c.gsh_orb_extract_batch_nostdlib(_ptr(imgs), w, h, n, _ptr(scoremaps), _ptr(kps), _ptr(counts), nkps,
                                              threshold)

    def orb_extract_pyramid_dev(self, img, buffer, nkps, threshold, n_levels):
        """nanomagick.c:245-290 on a device image; buffer: device bytes (levels + scoremaps)"""
        h, w = int(img.shape[0]), int(img.shape[1])
        kps = np.zeros(max(nkps, 1), KEYPOINT_DTYPE)
        n = self.c.gsh_orb_extract_pyramid(_ptr(img), w, h, _ptr(buffer), kps.ctypes.data, nkps, threshold,
                                           n_levels)
        return kps[:n].copy()

    def pyramid_batch(self, levels, imgs, n_levels):
        """gsh_pyramid_batch: levels 1 .. L-1 of the n frames of imgs (n, h, w) into `levels`, a flat uint8 device buffer
        of level planes (n frames each) back to back"""
        n, h, w = self._nhw(imgs)
        self.c.gsh_pyramid_batch(_ptr(levels), _ptr(imgs), w, h, n, n_levels)

    def orb_pyramid_batch_buffer_bytes(self, w, h, n_levels, n):
        return int(self.c.gsh_orb_pyramid_batch_buffer_bytes(w, h, n_levels, n))

    def orb_extract_pyramid_batch_nostdlib(self, imgs, buffer, kps, counts, nkps, threshold, n_levels, level_counts=None):
        """device-resident pyramid ORB (nanomagick.c:245-290, GS_NO_STDLIB trig): buffer orb_pyramid_batch_buffer_bytes
        uint8, kps (n, nkps, 12) int32, counts (n) and level_counts (n, 4) or None -- device tensors, nothing comes back
        to the host"""
        n, h, w = self._nhw(imgs)
        self.c.gsh_orb_extract_pyramid_batch_nostdlib(_ptr(imgs), w, h, n, _ptr(buffer), _ptr(kps), _ptr(counts),
                                                      _ptr(level_counts), nkps, threshold, n_levels)

    def orb_extract_pyramid_batch(self, imgs, buffer, kps, counts, nkps, threshold, n_levels, level_counts=None):
        """pyramid ORB of the reference's default build (nanomagick.c:245-290, glibc trig on the host): the arguments of
        orb_extract_pyramid_batch_nostdlib, device tensors; the records stay on the device, the call blocks for its one
        host round trip"""
        n, h, w = self._nhw(imgs)
        self.c.gsh_orb_extract_pyramid_batch(_ptr(imgs), w, h, n, _ptr(buffer), _ptr(kps), _ptr(counts),
                                             _ptr(level_counts), nkps, threshold, n_levels)

    def orb_pyramid_batch_times(self):
        """ms of the last orb_extract_pyramid_batch call under profile(True): device before, copy down, host trig, copy up,
        device after"""
        ms = (C.c_double * 5)()
        self.c.gsh_orb_pyramid_batch_times(ms)
        return list(ms)

    def orb_pyramid_buffer_fill_batch(self, buffer, single, w, h, n_levels, n):
        """gsh_orb_pyramid_buffer_fill_batch: every plane of the n frames of the batch buffer = that plane of `single`, one
        frame's buffer (orb_pyramid_buffer_bytes); flat uint8 device buffers"""
        self.c.gsh_orb_pyramid_buffer_fill_batch(_ptr(buffer), _ptr(single), w, h, n_levels, n)

    def match_orb_dev(self, k1, n1, k2, n2, matches, count, max_matches, max_distance):
        self.c.gsh_match_orb_dev(_ptr(k1), n1, _ptr(k2), n2, _ptr(matches), _ptr(count),
                                 max_matches, max_distance)

    @staticmethod
    def _keypoint_sets(k):
        """(cap, nset) of one (cap, 12) set of keypoint records or of nset sets (nset, cap, 12), int32"""
        if k.ndim not in (2, 3) or int(k.shape[-1]) != 12:
            raise ValueError("expected (cap, 12) or (nset, cap, 12) int32 keypoint records")
        return int(k.shape[-2]), (1 if k.ndim == 2 else int(k.shape[0]))

    def match_orb_batch(self, k1, n1, k2, n2, matches, counts, max_distance):
        """gsh_match_orb_batch: pair p of n = len(counts) = gs_match_orb of query set p of k1 -- or its one set -- against
        train set p of k2 -- or its one set; n1 / n2: per-set record counts (nset) read on the device, or None for all cap
        records; matches (n, max_matches, 3) int32 {idx1, idx2, distance}, counts (n) -- device tensors, nothing comes back
        to the host"""
        cap1, nset1 = self._keypoint_sets(k1)
        cap2, nset2 = self._keypoint_sets(k2)
        if matches.ndim != 3 or int(matches.shape[2]) != 3 or int(matches.shape[0]) != int(counts.shape[0]):
            raise ValueError("expected matches (n, max_matches, 3) and counts (n)")
        self.c.gsh_match_orb_batch(_ptr(k1), cap1, _ptr(n1), nset1, _ptr(k2), cap2, _ptr(n2), nset2, int(matches.shape[0]),
                                   _ptr(matches), _ptr(counts), int(matches.shape[1]), max_distance)

    def adaptive_threshold_batch(self, dst, src, radius, c):
        n, h, w = self._nhw(src)
        self.c.gsh_adaptive_threshold_batch(_ptr(dst), _ptr(src), w, h, n, radius, c)

    def filter_batch(self, dst, src, kernel, norm):
        n, h, w = self._nhw(src)
        k = np.ascontiguousarray(kernel).astype(np.int8)
        self.c.gsh_filter_batch(_ptr(dst), _ptr(src), w, h, n, k.ctypes.data, k.shape[1], k.shape[0],
                                norm)

    def downsample_batch(self, dst, src):
        n, h, w = self._nhw(src)
        self.c.gsh_downsample_batch(_ptr(dst), _ptr(src), w, h, n)

    def crop_batch(self, dst, src, x, y, w, h):
        """gsh_crop_batch: dst (n, h, w) = the window (x, y, w, h) of every frame of src (n, sh, sw) uint8"""
        n, sh, sw = self._nhw(src)
        self.c.gsh_crop_batch(_ptr(dst), _ptr(src), sw, sh, n, GsRect(x, y, w, h))

    def resize_batch(self, dst, src, nearest=False):
        """gsh_resize_batch / gsh_resize_nn_batch: dst (n, dh, dw) from src (n, sh, sw) uint8, frame by frame"""
        n, sh, sw = self._nhw(src)
        _, dh, dw = self._nhw(dst)
        (self.c.gsh_resize_nn_batch if nearest else self.c.gsh_resize_batch)(_ptr(dst), dw, dh, _ptr(src), sw, sh, n)

    def crop_resize_batch(self, dst, src, rois, frame_of=None, nearest=False):
        """gsh_crop_resize_batch: dst (npatches, dh, dw) uint8; patch p = the window rois[p] = (x, y, w, h) of frame
        frame_of[p] (frame p when frame_of is None) of src (n, sh, sw), resized; rois (npatches, 4) and frame_of
        (npatches) int32 device tensors, read on the device"""
        n, sh, sw = self._nhw(src)
        npatches, dh, dw = self._nhw(dst)
        self.c.gsh_crop_resize_batch(_ptr(dst), dw, dh, _ptr(src), sw, sh, n, _ptr(rois), _ptr(frame_of), npatches,
                                     1 if nearest else 0)

    @staticmethod
    def _templates(tmpl, n):
        """(tw, th, ntmpl) of one (th, tw) template for every frame or of n templates (n, th, tw)"""
        if tmpl.ndim == 2:
            return int(tmpl.shape[1]), int(tmpl.shape[0]), 1
        if tmpl.ndim != 3:
            raise ValueError("expected a (th, tw) or an (n, th, tw) uint8 template")
        return int(tmpl.shape[2]), int(tmpl.shape[1]), int(tmpl.shape[0])

    def match_template_batch(self, result, img, tmpl):
        """gsh_match_template_batch: result (n, ih - th + 1, iw - tw + 1) = gs_match_template of every frame of img
        (n, ih, iw) uint8 against tmpl (th, tw) -- one for all -- or tmpl (n, th, tw) -- template f for frame f"""
        n, ih, iw = self._nhw(img)
        tw, th, ntmpl = self._templates(tmpl, n)
        self.c.gsh_match_template_batch(_ptr(img), iw, ih, n, _ptr(tmpl), tw, th, ntmpl, _ptr(result))

    def find_best_match_batch(self, result, best, score=None):
        """gsh_find_best_match_batch: best (n, 2) int32 {x, y} = gs_find_best_match of every map of result (n, rh, rw)
        uint8, score (n) uint8 or None the map's value there -- device tensors, nothing comes back to the host"""
        n, rh, rw = self._nhw(result)
        self.c.gsh_find_best_match_batch(_ptr(result), rw, rh, n, _ptr(best), _ptr(score))

    def locate_template_batch(self, img, tmpl, best, score=None):
        """gsh_locate_template_batch: match_template_batch + find_best_match_batch without a result map"""
        n, ih, iw = self._nhw(img)
        tw, th, ntmpl = self._templates(tmpl, n)
        self.c.gsh_locate_template_batch(_ptr(img), iw, ih, n, _ptr(tmpl), tw, th, ntmpl, _ptr(best), _ptr(score))

    def match_templates_batch(self, result, img, tmpl):
        """gsh_match_templates_batch: result (n, m, ih - th + 1, iw - tw + 1) = gs_match_template of every frame of img
        (n, ih, iw) uint8 against every template of the bank tmpl (m, th, tw)"""
        n, ih, iw = img.shape
        m, th, tw = tmpl.shape
        self.c.gsh_match_templates_batch(_ptr(img), iw, ih, n, _ptr(tmpl), tw, th, m, _ptr(result))

    def locate_templates_batch(self, img, tmpl, best, score=None, winner=None):
        """gsh_locate_templates_batch: best (n, m, 2) int32 {x, y} and score (n, m) uint8 of match_templates_batch's maps without
        the maps; winner (n) int32: per frame the template with the highest score, the lowest index on ties"""
        n, ih, iw = img.shape
        m, th, tw = tmpl.shape
        self.c.gsh_locate_templates_batch(_ptr(img), iw, ih, n, _ptr(tmpl), tw, th, m, _ptr(best), _ptr(score), _ptr(winner))

    @staticmethod
    def _windows(windows, tmpl):
        """(nwin, tw, th, ntmpl): windows (nwin, 4) int32 / uint32 {x, y, w, h} or (nwin) RECT_DTYPE; tmpl (th, tw) -- one
        for all windows -- or (nwin, th, tw)"""
        nwin = int(windows.shape[0])
        if not (windows.ndim == 1 or (windows.ndim == 2 and int(windows.shape[1]) == 4)):
            raise ValueError("expected windows (nwin, 4) {x, y, w, h} or (nwin) RECT_DTYPE")
        tw, th, ntmpl = Grayskull._templates(tmpl, nwin)
        return nwin, tw, th, ntmpl

    def locate_template_windows_batch(self, img, tmpl, windows, max_size, best, score=None, frame_of=None):
        """gsh_locate_template_windows_batch: per window p = windows[p] (x, y, w, h in frame coordinates) of frame frame_of[p]
        (frame p when frame_of is None) of img (n, ih, iw) uint8, gs_find_best_match(gs_match_template(gs_crop(...), tmpl)):
        best (nwin, 2) uint32 / int32 {x, y} in FRAME coordinates, score (nwin) uint8 or None.  max_size = (max_ww, max_wh):
        the host's upper bound on a window's size.  An invalid window gets {0xFFFFFFFF, 0xFFFFFFFF} and score 0.  windows,
        frame_of, best and score live where img lives and are read and written there"""
        n, ih, iw = self._nhw(img)
        nwin, tw, th, ntmpl = self._windows(windows, tmpl)
        self.c.gsh_locate_template_windows_batch(_ptr(img), iw, ih, n, _ptr(tmpl), tw, th, ntmpl, _ptr(windows), _ptr(frame_of), nwin,
                                                 int(max_size[0]), int(max_size[1]), _ptr(best), _ptr(score))

    def match_template_windows_batch(self, result, img, tmpl, windows, max_size, frame_of=None):
        """gsh_match_template_windows_batch: result (nwin, max_wh - th + 1, max_ww - tw + 1) uint8 holds one SLOT per window;
        window p's map of (h - th + 1) rows of (w - tw + 1) bytes lies at the slot's start with row pitch w - tw + 1, the
        rest of the slot -- and the whole slot of an invalid window -- is left untouched"""
        n, ih, iw = self._nhw(img)
        nwin, tw, th, ntmpl = self._windows(windows, tmpl)
        self.c.gsh_match_template_windows_batch(_ptr(img), iw, ih, n, _ptr(tmpl), tw, th, ntmpl, _ptr(windows), _ptr(frame_of), nwin,
                                                int(max_size[0]), int(max_size[1]), _ptr(result))

    def search_windows_batch(self, at, box, margin, frame_size, windows):
        """gsh_search_windows_batch: windows (nwin, 4) = the box (at[p].x, at[p].y, box = (bw, bh)) grown by margin = (mx, my) on
        every side and clipped to the frame, frame_size = (iw, ih); at (nwin, 2) {x, y}, e.g. locate's best.  A point outside
        the frame -- locate's invalid sentinel -- gives (0, 0, 0, 0), an invalid window"""
        self.c.gsh_search_windows_batch(_ptr(at), int(at.shape[0]), int(box[0]), int(box[1]), int(margin[0]), int(margin[1]),
                                        int(frame_size[0]), int(frame_size[1]), _ptr(windows))

    def blobs_batch(self, img, labels, blobs, counts, nblobs):
        """gsh_blobs_batch: img (n, h, w) uint8, labels (n, h, w) uint16 [or int16], blobs (n, nblobs, 8) int32 (one
        32-byte record per row: see BLOB_DTYPE), counts (n) int32 -- all device tensors; stream-ordered"""
        n, h, w = self._nhw(img)
        self.c.gsh_blobs_batch(_ptr(img), w, h, n, _ptr(labels), _ptr(blobs), _ptr(counts), nblobs)

    def blob_corners_batch(self, img, labels, blobs, corners):
        """gsh_blob_corners_batch: blobs (n, 8) int32 -- one record per frame --, corners (n, 4, 2) int32"""
        n, h, w = self._nhw(img)
        self.c.gsh_blob_corners_batch(_ptr(img), _ptr(labels), w, h, n, _ptr(blobs), _ptr(corners))

    def perspective_correct_batch(self, dst, src, corners):
        """gsh_perspective_correct_batch: dst (n, dh, dw), src (n, sh, sw) uint8, corners (n, 4, 2) int32"""
        n, sh, sw = self._nhw(src)
        _, dh, dw = self._nhw(dst)
        self.c.gsh_perspective_correct_batch(_ptr(dst), dw, dh, _ptr(src), sw, sh, n, _ptr(corners))

    def blob_largest_batch(self, blobs, counts, largest, index=None):
        """gsh_blob_largest_batch: blobs (n, nblobs, 8) int32 and counts (n) int32 as blobs_batch left them; largest (n, 8)
        int32 receives each frame's first record of maximum area, index (n) int32 or None its position (-1: no blob)"""
        self.c.gsh_blob_largest_batch(_ptr(blobs), int(blobs.shape[1]), _ptr(counts), int(blobs.shape[0]), _ptr(largest),
                                      _ptr(index))

    def threshold_batch_dev_offset(self, img, thr, offset):
        """gsh_threshold_batch_dev_offset: frame f in place at (uint8_t)(thr[f] + offset); thr (n) uint8"""
        n, h, w = self._nhw(img)
        self.c.gsh_threshold_batch_dev_offset(_ptr(img), w, h, n, _ptr(thr), int(offset))

    def blob_paint_batch(self, dst, img, blobs, counts):
        """gsh_blob_paint_batch: dst, img (n, h, w) uint8, blobs (n, nblobs, 8) int32, counts (n) int32 -- the picture
        nanomagick's `blobs` verb draws, one per frame"""
        n, h, w = self._nhw(img)
        self.c.gsh_blob_paint_batch(_ptr(dst), _ptr(img), w, h, n, _ptr(blobs), int(blobs.shape[1]), _ptr(counts))

    def trace_contours_batch(self, img, visited, contours, counts=None, status=None):
        """gsh_trace_contours_batch: img, visited (n, h, w) uint8, contours (n, per_frame, 7) int32 (one 28-byte record
        per row: see CONTOUR_DTYPE; `start` read, box and length written), counts (n) int32 or None, status
        (n, per_frame) uint8 or None -- all device tensors; stream-ordered"""
        n, h, w = self._nhw(img)
        self.c.gsh_trace_contours_batch(_ptr(img), _ptr(visited), w, h, n, _ptr(contours), int(contours.shape[1]),
                                        _ptr(counts), _ptr(status))

    def blob_contour_starts_batch(self, labels, blobs, counts, contours):
        """gsh_blob_contour_starts_batch: labels (n, h, w) uint16 [or int16], blobs (n, nblobs, 8) int32, counts (n) int32
        or None as blobs_batch left them; contours (n, nblobs, 7) int32 receive each blob's raster-first pixel as start"""
        n, h, w = self._nhw(labels)
        self.c.gsh_blob_contour_starts_batch(_ptr(labels), w, h, n, _ptr(blobs), int(blobs.shape[1]), _ptr(counts),
                                             _ptr(contours))

    def synth_batch(self, dst, seed0):
        n, h, w = self._nhw(dst)
        self.c.gsh_synth_batch(_ptr(dst), w, h, n, seed0)

    def checksum_batch(self, img, sums):
        n = int(img.shape[0])
        frame_bytes = int(np.prod(img.shape[1:])) * (img.element_size() if hasattr(img, "element_size") else img.itemsize)
        self.c.gsh_checksum_batch(_ptr(img), frame_bytes, n, _ptr(sums))


class DeviceCascade:
    """cascade tables flattened into device memory (gsh_cascade_create)"""

    def __init__(self, gs, cascade):
        self._gs, self._keep = gs, cascade
        self.handle = gs.c.gsh_cascade_create(C.addressof(cascade.as_struct()))

    def close(self):
        if self.handle:
            self._gs.c.gsh_cascade_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default = None


def lib():
    """the process-wide binding of libgrayskull_hip.so (raises ImportError if not built)"""
    global _default
    if _default is None:
        _default = Grayskull()
    return _default


def __getattr__(name):  # gs.blur(...) == gs.lib().blur(...)
    if name.startswith("_"):
        raise AttributeError(name)
    return getattr(lib(), name)
