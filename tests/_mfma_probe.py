"""Test-side loader of the mfma_blocks.h probe libraries (tests/kernels/): ctypes and numpy only, no torch.

A launch hands `ncases` flat LDS images (float64, `words` each) and one parameter list to ONE routine of mfma_blocks.h and gets
every image back as the routine left it, with the routine's returned flag per case (tests/kernels/mfma_blocks_probe.hip)."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_DIR = os.path.join(ROOT, "tests", "kernels")
LIBRARIES = {"left": "libmfma_probe.so", "right": "libmfma_probe_rl.so", "fused": "libmfma_probe_fused.so"}
FORMS = {"left": b"left-looking", "right": b"right-looking", "fused": b"fused"}

# the op codes of mfma_blocks_probe.hip (enum ProbeOp)
(MMA_TILE, MMA_TILE2, MMA_TILE_2A, MMA_TILE_RB, CHOL16, CHOL16_MFMA, CHOL16_N4, CHOL16_N6, CHOL16_N8, CHOL16_N12, CHOL16_NC,
 CHOL_BLOCKED_WAVE, CHOL_BLOCKED, CHOL_TILES_WAVE, CHOL_TILES, CHOL_TILES_LAST6, CHOL_TILES_LAST12,
 TRSM_FWD_BLOCKED, TRSM_BWD_BLOCKED, TRSM_FWD_TILES, TRSM_BWD_TILES) = range(21)
CHOL16_N = {4: CHOL16_N4, 6: CHOL16_N6, 8: CHOL16_N8, 12: CHOL16_N12}
CHOL_TILES_LAST = {6: CHOL_TILES_LAST6, 12: CHOL_TILES_LAST12}
MAX_WORDS = (160 * 1024 - 64) // 8

_probes = {}
_gpu_error = None   # the first HIP error of this process: nothing more is started on the device after it


class Probe:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        self.lib.mfma_probe_run.argtypes = [ctypes.c_int] * 4 + [ip, ctypes.c_int, dp, dp, ip]
        self.lib.mfma_probe_run.restype = ctypes.c_int
        self.lib.mfma_probe_rsqrt.argtypes = [ctypes.c_int, dp, dp]
        self.lib.mfma_probe_rsqrt.restype = ctypes.c_int
        self.lib.mfma_probe_form.restype = ctypes.c_char_p
        self.lib.mfma_probe_error_string.argtypes = [ctypes.c_int]
        self.lib.mfma_probe_error_string.restype = ctypes.c_char_p
        self.form = self.lib.mfma_probe_form()

    def _check(self, err, what):
        global _gpu_error
        if err != 0:
            _gpu_error = _gpu_error or what
            raise RuntimeError("%s: hipError %d (%s)" % (what, err, self.lib.mfma_probe_error_string(err).decode()))

    def run(self, op, threads, params, images):
        """images: (ncases, words) float64 -> (images after the call, flags as bool (ncases,))"""
        if _gpu_error:
            raise RuntimeError("not launched: %s failed earlier in this process" % _gpu_error)
        images = np.ascontiguousarray(images, dtype=np.float64)
        assert images.ndim == 2 and 1 <= images.shape[1] <= MAX_WORDS, images.shape
        ncases, words = images.shape
        out = np.empty_like(images)
        flags = np.full(ncases, -1, dtype=np.int32)
        par = np.asarray(params, dtype=np.int32)
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        err = self.lib.mfma_probe_run(int(op), int(threads), ncases, words, par.ctypes.data_as(ip), par.size,
                                      images.ctypes.data_as(dp), out.ctypes.data_as(dp), flags.ctypes.data_as(ip))
        self._check(err, "mfma_probe_run(op %d)" % op)
        assert np.all((flags == 0) | (flags == 1)), flags
        return out, flags.astype(bool)

    def rsqrt_refined(self, x):
        if _gpu_error:
            raise RuntimeError("not launched: %s failed earlier in this process" % _gpu_error)
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        dp = ctypes.POINTER(ctypes.c_double)
        self._check(self.lib.mfma_probe_rsqrt(x.size, x.ctypes.data_as(dp), out.ctypes.data_as(dp)), "mfma_probe_rsqrt")
        return out


def _stale(path):
    if not os.path.exists(path):
        return True
    srcs = [os.path.join(KERNEL_DIR, "mfma_blocks_probe.hip"), os.path.join(KERNEL_DIR, "Makefile"),
            os.path.join(ROOT, "mpc_benchmark_amd", "csrc", "mfma_blocks.h"), os.path.join(ROOT, "mpc_benchmark_amd", "csrc", "device_common.h")]
    return any(os.path.getmtime(s) > os.path.getmtime(path) for s in srcs)


def load(build="left"):
    """The probe library of one build: 'left' (default flags, as mpc_hip.hip), 'right' (-DCHOL16_RIGHT_LOOKING, as eval_multibody.hip),
    'fused' (-DCHOL16_FUSED).  Built with make when missing or older than its sources."""
    if build not in _probes:
        # MFMA_PROBE_DIR: probe libraries built elsewhere (e.g. from a deliberately broken copy of the header, to see which test catches it)
        override = os.environ.get("MFMA_PROBE_DIR")
        path = os.path.join(override or KERNEL_DIR, LIBRARIES[build])
        if not override and _stale(path):
            try:
                subprocess.run(["make", "-s", "-C", KERNEL_DIR, LIBRARIES[build]], check=True)
            except Exception:
                if not os.path.exists(path):
                    raise
        probe = Probe(path)
        assert probe.form == FORMS[build], (build, probe.form)
        _probes[build] = probe
    return _probes[build]
