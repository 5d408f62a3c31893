"""The Gaussian / pyramid part of the reference ``features.py`` on the GPU.

* ``gaussian_filter(img, sigma=1.0)``  - features.py:20-24
* ``pyr_down`` / ``gaussian_pyramid``   - the ``cv2.pyrDown`` chain of the MSOP
  detector, features.py:138-155
* ``sift_pyramid(img)``                 - the Gaussian and difference-of-Gaussian
  scale space that ``sift_detector`` (features.py:192-201) gets from
  ``cv2.xfeatures2d.SIFT_create().detectAndCompute``.

All filters run in ``libpano360_hip.so`` (``pano_blur_plane``, ``pano_pyr_down``,
``pano_gray_u8``, ``pano_resize_up2``, ``pano_decimate2``, ``pano_scale_step``).
The SIFT arithmetic is inside OpenCV, not in the reference repo: its published
algorithm (SIFT defaults: sigma 1.6, 3 layers per octave, first octave -1) is
restated, parity unpinned.
* ``sift_detector()``                   - features.py:192-201: keypoints, 128-d
  descriptors (``pano_sift_extrema`` / ``_orient`` / ``_describe``) and the RootSIFT
  normalisation.
* ``flann_matching(des1, des2)``        - features.py:222-232: the 2-nearest-neighbour
  search and Lowe's 0.7 ratio test, exhaustive and exact on the GPU (``pano_knn2``:
  matrix-core cross terms rank the candidates, the winners are re-evaluated in float32)
  where the reference asks FLANN's randomised kd-trees for an approximate answer.
* ``find_homography(src, dst, RANSAC)``  - features.py:244, ``cv2.findHomography`` with
  ``cv2.RANSAC``: ``pano_hom_ransac`` scores every hypothesis of every pair of a batch on the
  GPU and refits the winner (a Hartley-normalised DLT; no adaptive stop, no Levenberg-Marquardt
  polish - include/pano360.h pins the contract).
* ``msop_detect`` / ``msop_detector`` / ``ssc`` / ``rot_mat`` - features.py:27-156, 204-212: the
  MSOP detector.  Harris corners (``pano_harris``), the cut of the strongest local maxima
  (``pano_msop_candidates``, ``pano_msop_cut``), the greedy walks of the adaptive non-maximal
  suppression (``pano_ssc_probe``; the scalar binary search around them stays in Python) and the
  oriented 8 x 8 descriptors (``pano_sobel``, ``pano_msop_smooth``, ``pano_msop_describe``).
  OpenCV's part restated, parity unpinned; DESIGN 5i states the arithmetic.
* ``matching(imgs)``, ``_match_hom``, ``_reverse`` - features.py:235-283: detection, 2-NN, the
  ratio test (``pano_match_pack``) and one RANSAC launch over every pair; ``main`` writes the
  ``matches_<name>.npz`` the reference's stitcher.py:423-428 loads.
"""
import argparse
import ctypes as C
import logging
import math
import os
import time
from collections import defaultdict

import numpy as np

from . import _lib
from . import engine as _eng

SIFT_SIGMA = 1.6            # cv2.xfeatures2d.SIFT_create() defaults
SIFT_LAYERS = 3
SIFT_INIT_SIGMA = 0.5


def _to_device(img):
    import torch
    eng = _eng.engine()
    return eng, torch.from_numpy(np.ascontiguousarray(img, np.float32)).to(eng.device)


def gaussian_filter(img, sigma=1.0):
    """Compute the kernel size from sigma and smooth the image
    (features.py:20-24): ksize = max(int((sigma-0.35)/0.15), 1), made odd."""
    ksz = max(int((sigma - 0.35) / 0.15), 1)
    ksz += not ksz % 2
    eng, dev = _to_device(img)
    if dev.ndim == 2:
        return eng.blur_plane(dev, ksz, sigma).cpu().numpy()
    planes = [eng.blur_plane(dev[..., c].contiguous(), ksz, sigma) for c in range(dev.shape[2])]
    import torch
    return torch.stack(planes, dim=-1).cpu().numpy()


def pyr_down(img):
    """``cv2.pyrDown`` of a float32 plane (features.py:155)."""
    eng, dev = _to_device(img)
    return eng.pyr_down(dev).cpu().numpy()


def gaussian_pyramid(img, levels=4):
    """The pyrDown chain the MSOP detector walks (features.py:138-155)."""
    eng, dev = _to_device(img)
    out = [dev]
    for _ in range(levels - 1):
        out.append(eng.pyr_down(out[-1]))
    return [p.cpu().numpy() for p in out]


# ------------------------------------------------------------- SIFT scale space
def sift_sigmas(sigma=SIFT_SIGMA, layers=SIFT_LAYERS):
    """Incremental sigmas of buildGaussianPyramid: sig[0] = sigma,
    sig[i] = sqrt((sigma k^i)^2 - (sigma k^(i-1))^2), k = 2^(1/layers)."""
    k = 2.0 ** (1.0 / layers)
    out = [sigma]
    for i in range(1, layers + 3):
        prev = k ** (i - 1) * sigma
        out.append(float(np.sqrt((prev * k) ** 2 - prev ** 2)))
    return out


def sift_octaves(height, width):
    """nOctaves of SIFT for a base image already doubled in size (first octave
    -1): cvRound(log2(min side of the doubled image) - 2) + 1."""
    return int(np.rint(np.log(float(min(2 * height, 2 * width))) / np.log(2.0) - 2)) + 1


class _Dev:
    """Thin typed wrappers over the pyramid entry points (device tensors)."""

    def __init__(self, eng):
        self.eng = eng

    def _new(self, h, w):
        import torch
        return torch.empty((h, w), dtype=torch.float32, device=self.eng.device)

    def gray(self, frame):
        h, w = frame.shape[:2]
        out = self._new(h, w)
        self.eng.call("pano_gray_u8", frame, h, w, out)
        return out

    def up2(self, plane):
        h, w = plane.shape
        out = self._new(2 * h, 2 * w)
        self.eng.call("pano_resize_up2", plane, h, w, out)
        return out

    def half(self, plane):
        h, w = plane.shape
        out = self._new(h // 2, w // 2)
        self.eng.call("pano_decimate2", plane, h, w, out)
        return out

    def sub(self, a, b):
        out = self._new(*a.shape)
        self.eng.call("pano_subtract", a, b, a.numel(), out)
        return out

    def blur(self, plane, sigma):
        return self.eng.blur_plane(plane, _eng.gaussian_ksize(sigma), sigma).contiguous()


_STEP_TAPS = {}


def _step_taps(sigma):
    """cv::getGaussianKernel(cvRound(8 sigma + 1) | 1, sigma) as a host float32 array."""
    key = float(sigma)
    if key not in _STEP_TAPS:
        _STEP_TAPS[key] = np.ascontiguousarray(_eng.gaussian_taps(_eng.gaussian_ksize(key), key))
    return _STEP_TAPS[key]


def sift_pyramid_device(frame, n_octaves=None, sigma=SIFT_SIGMA, layers=SIFT_LAYERS, eng=None):
    """Gaussian and DoG pyramids of a uint8 BGR frame already on the device.
    Returns (gauss, dog): lists over octaves of contiguous stacks
    [layers+3][h][w] / [layers+2][h][w] (index them like lists of planes).
    One native call (``pano_scale_space``) queues every launch of the frame; one launch per
    layer (``scale_step_kernel``) blurs layer i-1 into layer i - both passes, the row-pass
    image staying in LDS - and writes the DoG layer i-1 from the same tile.
    ``layers`` = 2 is refused (``PanoError``): its last step needs a 37-tap aperture
    (sigma 4.53), and ``pano_scale_step`` takes apertures up to 33."""
    import torch
    eng = eng or _eng.engine()
    h, w = (int(v) for v in frame.shape[:2])
    if n_octaves is None:
        n_octaves = sift_octaves(h, w)
    # createInitialImage: grey -> float -> 2x bilinear -> blur to sigma
    sig_diff = float(np.sqrt(max(np.float32(sigma) ** 2 - np.float32(SIFT_INIT_SIGMA) ** 2 * 4,
                                 np.float32(0.01))))
    kernels = [_step_taps(s) for s in [sig_diff] + sift_sigmas(sigma, layers)[1:]]
    dims, rows, cols = [], 2 * h, 2 * w
    for o in range(n_octaves):
        dims.append((rows, cols))
        if min(rows, cols) < 2:             # buildGaussianPyramid would halve it to nothing
            break
        rows, cols = rows // 2, cols // 2
    f32 = dict(dtype=torch.float32, device=eng.device)
    gauss = [torch.empty((layers + 3, r, c), **f32) for r, c in dims]
    dog = [torch.empty((layers + 2, r, c), **f32) for r, c in dims]
    work = torch.empty(5 * h * w, **f32)
    taps = np.ascontiguousarray(np.concatenate(kernels), np.float32)
    ntaps = (C.c_int * len(kernels))(*[len(k) for k in kernels])
    gptr = (C.c_void_p * len(dims))(*[g.data_ptr() for g in gauss])
    dptr = (C.c_void_p * len(dims))(*[d.data_ptr() for d in dog])
    eng.call("pano_scale_space", frame, h, w, len(dims), layers, taps, ntaps, gptr, dptr, work)
    return gauss, dog


# ------------------------------------------------------- SIFT keypoints, descriptors
SIFT_CONTRAST = 0.04        # cv2.xfeatures2d.SIFT_create() defaults
SIFT_EDGE = 10.0
SIFT_FIRST_OCTAVE = -1
KP_DTYPE = np.dtype(_lib.SiftKeypoint)
KP_BYTES = KP_DTYPE.itemsize


class KeyPoint:
    """The fields of ``cv2.KeyPoint`` the reference reads (features.py:223-232: ``pt``)."""
    __slots__ = ("pt", "size", "angle", "response", "octave", "class_id")

    def __init__(self, x, y, size, angle=-1.0, response=0.0, octave=0, class_id=-1):
        self.pt = (float(x), float(y))
        self.size, self.angle, self.response = float(size), float(angle), float(response)
        self.octave, self.class_id = int(octave), int(class_id)

    def __repr__(self):
        return (f"KeyPoint(pt=({self.pt[0]:.2f}, {self.pt[1]:.2f}), size={self.size:.2f}, "
                f"angle={self.angle:.1f}, octave={self.octave})")


def sift_sort_unique(kps):
    """KeyPointsFilter::removeDuplicatedSorted on a KP_DTYPE array: order by x, y,
    size (descending), angle, response (descending), octave (descending); keep the
    first of keypoints that share x, y, size and angle."""
    order = np.lexsort((-kps["octave"].astype(np.int64), -kps["response"], kps["angle"],
                        -kps["size"], kps["y"], kps["x"]))
    kps = kps[order]
    if len(kps) > 1:
        same = ((kps["x"][1:] == kps["x"][:-1]) & (kps["y"][1:] == kps["y"][:-1]) &
                (kps["size"][1:] == kps["size"][:-1]) & (kps["angle"][1:] == kps["angle"][:-1]))
        kps = kps[np.concatenate([[True], ~same])]
    return kps


class _SiftHost:
    """Per-engine host side of the detector: the copy stream, the pinned staging buffer of
    the keypoints and a ring of pinned counter slots.  Engines (one per host thread) share
    nothing; a lock orders the detections of one engine that finish from several threads."""

    SLOTS = 16

    def __init__(self, eng):
        import threading
        import torch
        self.lock = threading.Lock()
        self.side = torch.cuda.Stream(eng.device)
        self.pinned = None
        self.counts = torch.empty((self.SLOTS, 3), dtype=torch.int32).pin_memory()
        self.slot_events = [None] * self.SLOTS
        self.slot_gens = [0] * self.SLOTS        # hand-outs of each slot: whose counts it holds
        self.next = 0

    def counter_slot(self):
        """(slot, its generation, a pinned int32[3] that no queued copy still writes)."""
        with self.lock:
            k = self.next
            self.next = (k + 1) % self.SLOTS
            if self.slot_events[k] is not None:
                self.slot_events[k].synchronize()
            self.slot_gens[k] += 1
            return k, self.slot_gens[k], self.counts[k]

    def staging(self, nbytes):
        import torch
        if self.pinned is None or self.pinned.numel() < nbytes:
            self.pinned = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
        return self.pinned


def _sift_host(eng):
    host = getattr(eng, "_sift_host", None)
    if host is None:
        host = eng._sift_host = _SiftHost(eng)
    return host


class SiftDetection:
    """A ``detectAndCompute`` queued on the device: nothing has been waited for yet.
    ``result()`` waits, checks the counters and returns (keypoints as a KP_DTYPE array in
    OpenCV's order, descriptors float32 [K][128] on the device, values 0..255).

    ``ring`` = (workspace, its generation when this frame was queued) for a frame in a workspace of
    a ``SiftPipeline``: ``result()`` raises ``PanoError`` if a later frame has taken the workspace
    before it.  ``owned``: the descriptors returned are a copy of the caller's own, not a view into
    the workspace."""

    def __init__(self, counts, kpts, desc, max_keypoints, keep, eng, ring=None, owned=False):
        import torch
        self.counts, self.kpts, self.desc, self.max_keypoints = counts, kpts, desc, max_keypoints
        self.keep = keep                    # buffers the queued kernels still read
        self.ring, self.owned = ring, owned
        self._out = None
        self.host = _sift_host(eng)
        # the counters travel to pinned memory (a slot of the engine's ring) behind this frame's
        # kernels; `done` marks that point, so result() waits for THIS frame only, not for
        # whatever was queued after it
        self.slot, self.slot_gen, self.host_counts = self.host.counter_slot()
        self.host_counts.copy_(counts, non_blocking=True)
        self.stream = torch.cuda.current_stream(counts.device)
        self.done = torch.cuda.Event()
        self.done.record(self.stream)
        self.host.slot_events[self.slot] = self.done

    def result(self):
        import torch
        if self._out is None:
            if self.ring is not None and self.ring[0]["gen"] != self.ring[1]:
                raise _lib.PanoError("sift: the detection's workspace went to a later frame before "
                                     "its result() was taken (a SiftPipeline keeps `depth` frames)")
            self.done.synchronize()
            with self.host.lock:
                recycled = self.host.slot_gens[self.slot] != self.slot_gen
                counts = None if recycled else self.host_counts.numpy().copy()
            if recycled:
                # the pinned slot holds a later frame's counters now; the device's are still this
                # frame's (its workspace has not been taken, checked above)
                counts = self.counts.cpu().numpy()
            n_cand, n_kp, n_out = (int(v) for v in counts)
            if max(n_cand, n_kp) > self.max_keypoints:
                raise _lib.PanoError(f"sift: {max(n_cand, n_kp)} keypoints exceed max_keypoints")
            # the keypoints on a stream of their own: a copy on the compute stream would queue
            # behind the next frame's kernels.  One staging buffer per engine: the lock keeps
            # two results of this engine from sharing it
            with self.host.lock:
                pinned = self.host.staging(n_out * KP_BYTES)
                with torch.cuda.stream(self.host.side):   # pinned: a DMA, no staging kernel
                    pinned[:n_out * KP_BYTES].copy_(self.kpts[:n_out * KP_BYTES], non_blocking=True)
                self.host.side.synchronize()
                kps = pinned[:n_out * KP_BYTES].numpy().view(KP_DTYPE).copy()
            desc = self.desc[:n_out]
            if self.owned:
                desc = desc.clone()
                # a later frame queued on the detection's stream must not take the workspace
                # before the copy has read it
                cur = torch.cuda.current_stream(desc.device)
                if cur != self.stream:
                    self.stream.wait_stream(cur)
            self._out = (kps, desc)
            self.keep = None
        return self._out


class SiftPipeline:
    """Frames of ONE size through the detector's front end on one engine, a native call per frame
    (``pano_sift_detect``: scale space, extrema, orientations, OpenCV's order, descriptors - about
    110 launches - queued from C++ and, from the second frame of a set of buffers on, replayed as
    ONE HIP graph).  A graph holds addresses, so every buffer of a frame - the pyramid, the
    keypoint lists, the descriptors - lives in one of ``depth`` workspaces used in turn: what
    ``pyramid()`` / ``detect()`` hand back stays valid until ``depth`` more frames have been queued
    on this pipeline.  A detection's ``result()`` taken later raises ``PanoError``; the
    descriptors it returned earlier are a view into the workspace and are overwritten then (the
    keypoints are a host copy and stay).  ``owned``: ``result()`` returns a copy of the
    descriptors, the caller's to keep (the engine's own pipelines behind ``sift_detect_async``)."""

    def __init__(self, eng, h, w, depth=3, max_keypoints=1 << 18, n_octaves=None,
                 sigma=SIFT_SIGMA, layers=SIFT_LAYERS, owned=False):
        import torch
        self.eng, self.h, self.w, self.depth = eng, int(h), int(w), max(int(depth), 1)
        self.owned = bool(owned)
        self.max_keypoints, self.layers, self.sigma = int(max_keypoints), layers, sigma
        if n_octaves is None:
            n_octaves = sift_octaves(self.h, self.w)
        sig_diff = float(np.sqrt(max(np.float32(sigma) ** 2 - np.float32(SIFT_INIT_SIGMA) ** 2 * 4,
                                     np.float32(0.01))))
        kernels = [_step_taps(s) for s in [sig_diff] + sift_sigmas(sigma, layers)[1:]]
        self.taps = np.ascontiguousarray(np.concatenate(kernels), np.float32)
        self.ntaps = (C.c_int * len(kernels))(*[len(k) for k in kernels])
        self.dims, rows, cols = [], 2 * self.h, 2 * self.w
        for _ in range(n_octaves):
            self.dims.append((rows, cols))
            if min(rows, cols) < 2:         # buildGaussianPyramid would halve it to nothing
                break
            rows, cols = rows // 2, cols // 2
        self.slots, self.next = [], 0
        self._torch = torch

    def _slot(self):
        """The next workspace in turn (made on first use: 2.3 GB for a 4K frame)."""
        torch, eng, dev = self._torch, self.eng, self.eng.device
        k = self.next % self.depth
        self.next += 1
        if k < len(self.slots):
            return self.slots[k]
        f32 = dict(dtype=torch.float32, device=dev)
        ws = {}
        ws["gauss"] = [torch.empty((self.layers + 3, r, c), **f32) for r, c in self.dims]
        ws["dog"] = [torch.empty((self.layers + 2, r, c), **f32) for r, c in self.dims]
        ws["work"] = torch.empty(5 * self.h * self.w, **f32)
        ws["frame"] = torch.empty((self.h, self.w, 3), dtype=torch.uint8, device=dev)
        n = self.max_keypoints
        ws["cands"] = torch.empty(n * KP_BYTES, dtype=torch.uint8, device=dev)
        ws["kpts"] = torch.empty(n * KP_BYTES, dtype=torch.uint8, device=dev)
        ws["counts"] = torch.zeros(3, dtype=torch.int32, device=dev)
        ws["sort"] = torch.empty(int(eng.lib.pano_sift_sort_work_bytes(n)), dtype=torch.uint8,
                                 device=dev)
        ws["desc"] = torch.empty((n, 128), **f32)
        ws["gptr_host"] = (C.c_void_p * len(self.dims))(*[g.data_ptr() for g in ws["gauss"]])
        ws["dptr_host"] = (C.c_void_p * len(self.dims))(*[d.data_ptr() for d in ws["dog"]])
        # 256 entries each - one per value of a keypoint's octave byte, zeros beyond the pyramid:
        # a keypoint record that is not this frame's (octave byte 255 after the first-octave
        # adjustment) then finds an empty plane and samples nothing instead of a wild address
        dims_tab = np.zeros((256, 2), np.int32)
        dims_tab[:len(self.dims)] = self.dims
        gptr_tab = np.zeros(256, np.int64)
        gptr_tab[:len(self.dims)] = [g.data_ptr() for g in ws["gauss"]]
        ws["dims_dev"] = torch.from_numpy(dims_tab.reshape(-1)).to(dev)
        ws["gptr_dev"] = torch.from_numpy(gptr_tab).to(dev)
        a = _lib.SiftArgs()
        a.frame_copy = ws["frame"].data_ptr()
        a.h, a.w, a.n_octaves, a.n_layers = self.h, self.w, len(self.dims), self.layers
        a.taps, a.ntaps = self.taps.ctypes.data, C.cast(self.ntaps, C.c_void_p)
        a.gauss, a.dog = C.cast(ws["gptr_host"], C.c_void_p), C.cast(ws["dptr_host"], C.c_void_p)
        a.work = ws["work"].data_ptr()
        a.contrast_thr, a.edge_thr, a.sigma = SIFT_CONTRAST, SIFT_EDGE, self.sigma
        a.first_octave, a.max_keypoints = SIFT_FIRST_OCTAVE, n
        a.gauss_dev, a.dims_dev = ws["gptr_dev"].data_ptr(), ws["dims_dev"].data_ptr()
        a.cands, a.kpts = ws["cands"].data_ptr(), ws["kpts"].data_ptr()
        a.counts, a.sort_work, a.desc = (ws["counts"].data_ptr(), ws["sort"].data_ptr(),
                                         ws["desc"].data_ptr())
        ws["args"] = a
        ws["gen"] = 0                       # frames queued in this workspace
        self.slots.append(ws)
        return ws

    def _queue(self, frame, detect):
        if tuple(frame.shape) != (self.h, self.w, 3) or not frame.is_contiguous():
            raise ValueError(f"SiftPipeline of {self.h} x {self.w} frames got {tuple(frame.shape)}")
        ws = self._slot()
        ws["gen"] += 1                      # what a detection from this workspace held is gone
        a = ws["args"]
        a.frame, a.detect = frame.data_ptr(), 1 if detect else 0
        self.eng.call("pano_sift_detect", C.byref(a))
        ws["last_frame"] = frame            # (queued kernels read it)
        return ws

    @property
    def replaying(self):
        """True once the frames of the workspace used last go out as one graph launch."""
        return bool(self.eng.lib.pano_sift_detect_replaying(self.eng._ctx))

    def pyramid(self, frame):
        """(gauss, dog) of ``sift_pyramid_device``, in this pipeline's buffers."""
        ws = self._queue(frame, False)
        return ws["gauss"], ws["dog"]

    def detect(self, frame):
        """A queued ``detectAndCompute``: ``SiftDetection`` (``result()`` waits)."""
        ws = self._queue(frame, True)
        det = SiftDetection(ws["counts"], ws["cands"], ws["desc"], self.max_keypoints, (ws,), self.eng,
                            ring=(ws, ws["gen"]), owned=self.owned)
        det.pyramid = (ws["gauss"], ws["dog"])
        return det


def _pipeline_for(eng, h, w, max_keypoints):
    """The engine's pipeline for frames of this size (a few sizes are kept)."""
    kept = getattr(eng, "_sift_pipelines", None)
    if kept is None:
        kept = eng._sift_pipelines = {}
    key = (int(h), int(w), int(max_keypoints))
    if key not in kept:
        if len(kept) >= 2:
            kept.pop(next(iter(kept)))
        kept[key] = SiftPipeline(eng, h, w, depth=3, max_keypoints=max_keypoints, owned=True)
    return kept[key]


def sift_detect_async(frame, max_keypoints=1 << 18, pyramid=None, eng=None):
    """detectAndCompute of a uint8 BGR frame on the device, queued without a single wait: the
    candidate and keypoint counts stay on the device (``n_dev`` of ``pano_sift_sort_unique`` /
    ``pano_sift_describe``), so consecutive frames follow each other on the GPU.  (With a wait
    for every counter a 4K frame took 12.4 ms for 7.1 ms of kernels.)  ``pyramid`` =
    (gauss, dog) device stacks replaces the scale space of ``frame``; its layers per octave
    (DoG depth - 2, ``sift_pyramid_device(layers=...)``) are searched, ``ValueError`` if the
    octaves do not agree on them."""
    import torch
    eng = eng or _eng.engine()
    lib = eng.lib
    if pyramid is None:
        # the whole frame in one native call (a HIP graph from the second frame of a workspace on)
        # on the engine's pipeline of this frame size: take the result() before three more frames of
        # this size are queued on the engine (it raises after); the descriptors it returns are a
        # copy, the caller's to keep
        h, w = (int(v) for v in frame.shape[:2])
        return _pipeline_for(eng, h, w, max_keypoints).detect(frame.contiguous())
    gauss, dog = pyramid
    dev = eng.device
    # the layers per octave are the pyramid's: DoG depth - 2 (sift_pyramid_device(layers=...))
    n_layers = int(dog[0].shape[0]) - 2
    if n_layers < 1 or len(gauss) != len(dog) or any(
            int(d.shape[0]) != n_layers + 2 or int(g.shape[0]) != n_layers + 3
            for g, d in zip(gauss, dog)):
        raise ValueError("sift_detect_async: the pyramid's octaves must hold n + 3 Gaussian and "
                         "n + 2 DoG layers, the same n in every octave")
    # 256 entries each, zeros beyond the pyramid, as SiftPipeline._slot builds them: a record
    # whose octave byte is not this pyramid's finds an empty plane and samples nothing
    dims_host = np.zeros((256, 2), np.int32)
    dims_host[:len(gauss)] = [tuple(g.shape[1:]) for g in gauss]
    gptr_host = np.zeros(256, np.int64)
    gptr_host[:len(gauss)] = [g.data_ptr() for g in gauss]
    dims = eng.to_device(dims_host.reshape(-1)).view(torch.int32)
    gptr = eng.to_device(gptr_host).view(torch.int64)
    cands = torch.empty(max_keypoints * KP_BYTES, dtype=torch.uint8, device=dev)
    kpts = torch.empty(max_keypoints * KP_BYTES, dtype=torch.uint8, device=dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)    # candidates, keypoints, kept
    for o, diff in enumerate(dog):
        _, oh, ow = diff.shape
        eng.call("pano_sift_extrema", diff, oh, ow, o, n_layers, SIFT_CONTRAST, SIFT_EDGE,
                 SIFT_SIGMA, cands, counts[0:], max_keypoints)
    eng.call("pano_sift_orient", gptr, dims, n_layers, cands, counts[0:], max_keypoints, kpts,
             counts[1:], max_keypoints)
    # OpenCV's order and duplicate removal, and the first-octave adjustment (positions and
    # sizes halved, octave byte shifted: sift.cpp, detectAndCompute), on the device: the
    # six-key lexsort took 54 of a 4K frame's 69 ms on the host.  The capacity is sorted; the
    # slots past the device-side count sort to the end.
    work = torch.empty(int(lib.pano_sift_sort_work_bytes(max_keypoints)), dtype=torch.uint8,
                       device=dev)
    eng.call("pano_sift_sort_unique", kpts, max_keypoints, counts[1:], SIFT_FIRST_OCTAVE, work,
             cands, counts[2:])                              # cands: free again, reused as output
    desc = torch.empty((max_keypoints, 128), dtype=torch.float32, device=dev)
    eng.call("pano_sift_describe", gptr, dims, SIFT_FIRST_OCTAVE, cands, max_keypoints,
             counts[2:], desc)
    return SiftDetection(counts, cands, desc, max_keypoints, (gauss, dog, dims, gptr, kpts, work),
                         eng)


def sift_detect_device(frame, max_keypoints=1 << 18, pyramid=None, eng=None):
    """``sift_detect_async(...).result()``."""
    return sift_detect_async(frame, max_keypoints, pyramid, eng).result()


def sift_detector(eng=None):
    """Closure, return a SIFT detecting function (features.py:192-201):
    ``_detect(img) -> (keypoints, RootSIFT descriptors)``.  ``eng``: the engine to detect on
    (default: the process-wide one)."""
    def _detect(img):
        eng_ = eng if eng is not None else _eng.engine()
        frame = eng_.upload_frames([img])[0]
        kps, desc = sift_detect_device(frame, eng=eng_)
        des = desc.cpu().numpy()
        des = np.sqrt(des / (des.sum(axis=1, keepdims=True) + 1e-7))  # RootSIFT
        kp_ = [KeyPoint(k["x"], k["y"], k["size"], k["angle"], k["response"], k["octave"])
               for k in kps]
        return kp_, des

    return _detect


def sift_pyramid(img, n_octaves=None):
    """Host convenience: uint8 BGR image -> (gauss, dog) as NumPy arrays."""
    eng = _eng.engine()
    frame = eng.upload_frames([img])[0]
    gauss, dog = sift_pyramid_device(frame, n_octaves)
    to_np = lambda pyr: [[p.cpu().numpy() for p in octave] for octave in pyr]   # noqa: E731  (stacks iterate as planes)
    return to_np(gauss), to_np(dog)


# ------------------------------------------------------------------ MSOP detector
DSIZE = 8                   # features.py:16: descriptor size
MSOP_MAX_FEAT = (5000, 100, 25, 10)
HARRIS_K = 0.04             # features.py:140
SSC_PATHS = {"auto": _lib.SSC_AUTO, "onchip": _lib.SSC_ONCHIP, "global": _lib.SSC_GLOBAL}


def rot_mat(theta, pp_):
    """The 3 x 3 float32 matrix that turns by ``theta`` about the origin and then moves the origin
    to the point ``pp_`` = (row, col), in (x, y) order (features.py:102-106)."""
    row, col = pp_[0], pp_[1]
    turn = np.eye(3, dtype=np.float32)
    turn[0, 0] = turn[1, 1] = np.cos(theta)
    turn[0, 1] = np.sin(theta)
    turn[1, 0] = -turn[0, 1]
    turn[0, 2], turn[1, 2] = col, row
    return turn


class _SscSearch:
    """The scalar control of ``ssc``'s binary search (features.py:36-69, 91-97) in Python float64
    and Python ``round``: ``next_width()`` is the width to probe, None once the search is over;
    ``report(count)`` takes what the probe selected.  ``im_size`` is handed (H, W) and, as in the
    reference, its first entry is used as the number of columns."""

    def __init__(self, n_keypoints, im_size, n_points, tol=0.1):
        n_points = int(n_points)
        if n_points == 1:
            raise ValueError("ssc: n_points = 1 divides by zero in the search range")
        self.cols, self.rows = int(im_size[0]), int(im_size[1])
        # The widest suppression square that still lets n_points squares into the image (Bailo et
        # al., "Efficient adaptive non-maximal suppression algorithms for homogeneous spatial
        # keypoint distribution") is a root of  qa w^2 + qb w + qc = 0.  The coefficients and the
        # discriminant are exact integers; float64 enters at the square root.
        qa = n_points - 1
        qb = 2 * (self.rows + self.cols + 2 * n_points)
        qc = 4 * (n_points + self.cols - self.rows * self.cols)
        spread = math.sqrt(qb * qb - 4 * qa * qc)
        self.high = max(-round((qb + spread) / (2 * qa)), -round((qb - spread) / (2 * qa)))
        self.low = math.floor(math.sqrt(n_keypoints / n_points))
        slack = n_points * tol
        self.k_min, self.k_max = round(n_points - slack), round(n_points + slack)
        self.prev_width, self.complete, self.width = -1, False, None

    def next_width(self):
        if self.complete or self.low > self.high:
            return None
        width = self.low + (self.high - self.low) / 2
        if width == self.prev_width:
            return None
        self.width = width
        return width

    def grid(self):
        """(cgr, cell rows - 1, cell columns - 1, reach in cells) for the width to probe."""
        cgr = self.width / 2
        return (cgr, int(math.floor(self.rows / cgr)), int(math.floor(self.cols / cgr)),
                int(math.floor(self.width / cgr)))

    def report(self, count):
        if self.k_min <= count <= self.k_max:
            self.complete = True
        elif count < self.k_min:
            self.high = self.width - 1
        else:
            self.low = self.width + 1
        self.prev_width = self.width


def ssc_device(points, im_size, n_points, tol=0.1, eng=None, path="auto"):
    """``ssc`` over device points int32 [n][2] = (row, col): (indices int32 [n] on the device,
    how many of them count), the selection of the last probe that ran, in walk order.  Every
    probe is one launch of ``pano_ssc_probe`` and one 4-byte readback of its count; the search
    between them is ``_SscSearch``.  ``path``: "auto" | "onchip" | "global" (the coverage bitmap in
    LDS or in device memory, sized from the probe's width)."""
    import torch
    eng = eng or _eng.engine()
    n = int(points.shape[0])
    search = _SscSearch(n, im_size, n_points, tol)
    sel = torch.empty(max(n, 1), dtype=torch.int32, device=eng.device)
    count = torch.zeros(1, dtype=torch.int32, device=eng.device)
    taken = 0
    while search.next_width() is not None:
        cgr, ncr, ncc, reach = search.grid()
        onchip = (ncr + 1) * (ncc + 1) <= _lib.SSC_ONCHIP_CELLS
        work = None
        if path == "global" or (path == "auto" and not onchip):
            work = torch.empty(int(eng.lib.pano_ssc_probe_work_bytes(ncr, ncc)), dtype=torch.uint8,
                               device=eng.device)
        eng.call("pano_ssc_probe", points, n, cgr, ncr, ncc, reach, SSC_PATHS[path], work, sel,
                 count)
        taken = int(count.cpu()[0])
        search.report(taken)
    return sel, taken


def ssc(keypoints, im_size, n_points, tol=0.1, path="auto"):
    """Fast adaptive non-maximal suppression (features.py:27-99) of host keypoints, integer
    ``(kpt[0], kpt[1])`` inside ``im_size``; returns the list of the keypoints selected.  The
    walks run on the GPU (``ssc_device``)."""
    import torch
    kps = np.asarray(keypoints)
    if len(kps) == 0:
        return []
    pts = np.asarray(kps[:, :2], np.int64)
    if not np.array_equal(pts, np.asarray(kps[:, :2], np.float64)):
        raise ValueError("ssc: keypoints must hold integer positions")
    if pts.min() < 0 or pts[:, 0].max() >= im_size[0] or pts[:, 1].max() >= im_size[1]:
        raise ValueError("ssc: a keypoint lies outside im_size")
    eng = _eng.engine()
    dev = torch.from_numpy(np.ascontiguousarray(pts, np.int32)).to(eng.device)
    sel, taken = ssc_device(dev, im_size, n_points, tol, eng, path)
    return [keypoints[i] for i in sel[:taken].cpu().numpy()]


_SMOOTH_TAPS = {}


def _msop_smooth(eng, plane, sigma, tmp, out):
    """``gaussian_filter(plane, sigma)`` (features.py:20-24) of a dense device plane into ``out``
    by ``pano_msop_smooth``: OpenCV's operation order without FMA, where ``pano_blur_plane``
    spends one FMA per tap and differs in the last bit."""
    h, w = (int(v) for v in plane.shape)
    if sigma not in _SMOOTH_TAPS:
        ksz = max(int((sigma - 0.35) / 0.15), 1)
        ksz += not ksz % 2
        _SMOOTH_TAPS[sigma] = np.ascontiguousarray(_eng.gaussian_taps(ksz, sigma))
    taps = _SMOOTH_TAPS[sigma]
    eng.call("pano_msop_smooth", plane, h, w, taps, len(taps), tmp, out)
    return out


def msop_detect_device(frame, max_feat=MSOP_MAX_FEAT, eng=None, want_stages=False):
    """``msop_detect`` (features.py:133-156) of a uint8 BGR frame on the device: (points float64
    [N][4] = (scale row, scale col, theta, scale), descs float32 [N][64]), both on the device.
    Per level: ``pano_harris``, ``pano_msop_candidates`` (one readback: their count),
    ``pano_msop_cut``, ``ssc_device``, ``pano_sobel`` + ``pano_msop_smooth`` for the gradient and the
    blurred plane, ``pano_msop_describe``, ``pano_pyr_down``.  ``want_stages``: also a list with,
    per level, a dict of the response ``hrs``, the cut's ``cut`` (row, col), the ``sel`` indices
    of ``ssc``, ``g_x``, ``g_y``, ``blurred``, ``theta`` and the raw ``tiles``.  ``ValueError``
    when a level is left without points or asks for a single one (the reference fails there)."""
    import torch
    eng = eng or _eng.engine()
    lib, dev = eng.lib, eng.device
    frame = frame.contiguous()
    gray = _Dev(eng).gray(frame)
    points, descs, stages = [], [], []
    for lvl, maxf in enumerate(max_feat):
        maxf = int(maxf)
        h, w = (int(v) for v in gray.shape)
        hrs = torch.empty_like(gray)
        eng.call("pano_harris", gray, h, w, HARRIS_K, hrs)
        keys = torch.empty(h * w, dtype=torch.int32, device=dev)
        pos = torch.empty(h * w, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        work = torch.empty(int(lib.pano_msop_candidates_work_bytes(h, w)), dtype=torch.uint8,
                           device=dev)
        eng.call("pano_msop_candidates", hrs, h, w, work, keys, pos, count)
        n_cand = int(count.cpu()[0])
        keep = min(n_cand, 20 * maxf)
        if keep == 0:
            raise ValueError(f"msop_detect: level {lvl} has no candidates")
        cut = torch.empty((keep, 2), dtype=torch.int32, device=dev)
        work = torch.empty(int(lib.pano_msop_cut_work_bytes(n_cand)), dtype=torch.uint8, device=dev)
        eng.call("pano_msop_cut", keys, pos, n_cand, keep, w, work, cut)
        sel, taken = ssc_device(cut, (h, w), maxf, eng=eng)
        if taken == 0:
            raise ValueError(f"msop_detect: ssc left level {lvl} without points")
        d_x, d_y = torch.empty_like(gray), torch.empty_like(gray)
        eng.call("pano_sobel", gray, h, w, d_x, d_y)
        tmp = torch.empty_like(gray)
        g_x = _msop_smooth(eng, d_x, 1.0, tmp, d_x)           # gaussian_filter(.., 1.0): ksize 5
        g_y = _msop_smooth(eng, d_y, 1.0, tmp, d_y)
        blurred = _msop_smooth(eng, gray, 2.0, tmp, torch.empty_like(gray))   # ksize 11
        pts = torch.empty((taken, 4), dtype=torch.float64, device=dev)
        theta = torch.empty(taken, dtype=torch.float32, device=dev)
        tiles = torch.empty((taken, DSIZE, DSIZE), dtype=torch.float32, device=dev) \
            if want_stages else None
        desc = torch.empty((taken, DSIZE * DSIZE), dtype=torch.float32, device=dev)
        eng.call("pano_msop_describe", g_x, g_y, blurred, h, w, cut, sel, taken, 2 ** lvl, pts,
                 theta, tiles, desc)
        points.append(pts)
        descs.append(desc)
        if want_stages:
            stages.append({"hrs": hrs, "cut": cut, "sel": sel[:taken], "g_x": g_x, "g_y": g_y,
                           "blurred": blurred, "theta": theta, "tiles": tiles})
        if lvl + 1 < len(max_feat):
            gray = eng.pyr_down(gray)
    out = (torch.cat(points), torch.cat(descs))
    return out + (stages,) if want_stages else out


def msop_detect(img, max_feat=MSOP_MAX_FEAT):
    """Extract MSOP features (features.py:133-156): (points float64 [N][4], descs float32
    [N][64]) on the host."""
    eng = _eng.engine()
    frame = eng.upload_frames([img])[0]
    points, descs = msop_detect_device(frame, max_feat, eng)
    return points.cpu().numpy(), descs.cpu().numpy()


def msop_detector(max_feat=MSOP_MAX_FEAT, eng=None):
    """Closure, returns a MSOP detector (features.py:204-212): ``_detect(img) -> (keypoints,
    descriptors [N][64])``.  As there, a keypoint's ``size`` carries theta."""
    def _detect(img):
        eng_ = eng if eng is not None else _eng.engine()
        frame = eng_.upload_frames([img])[0]
        points, des = msop_detect_device(frame, max_feat, eng_)
        kp_ = [KeyPoint(p[1], p[0], p[2]) for p in points.cpu().numpy()]
        return kp_, des.cpu().numpy().reshape(-1, 64)

    return _detect


def detector_kwargs(name):
    """``matching``'s keyword for the command line's ``--detector``: none for "sift" (the
    default detector stays what it is)."""
    if name == "sift":
        return {}
    if name == "msop":
        return {"detect": msop_detector()}
    raise ValueError(f"detector {name!r} (sift or msop)")


# ------------------------------------------------------------------ matching
class DMatch:
    """The fields of ``cv2.DMatch`` the reference reads (features.py:238)."""
    __slots__ = ("queryIdx", "trainIdx", "distance")

    def __init__(self, query, train, distance):
        self.queryIdx, self.trainIdx, self.distance = int(query), int(train), float(distance)


def _knn_scale(peak):
    """A power of two that brings the largest magnitude of both sets into (512, 1024]: inside
    the interval ``pano_knn2`` states for it (at most 2048, and the train set's largest times the
    scale at least 2^-3) whenever the train set's peak is within 2^12 of the joint one, as the
    descriptors of one detector are (DESIGN, "The scale rule of pano_knn2")."""
    return float(2.0 ** np.floor(np.log2(1024.0 / peak))) if peak > 0 else 1.0


def knn2_device(des1, des2, eng=None, want_rescans=False, scale=None):
    """Two nearest rows of ``des2`` (Euclidean) for every row of ``des1``; both device
    float32 [K][D], D <= 128.  Returns (indices int64 [K1][2], distances float32 [K1][2]),
    nearest first.  ``pano_knn2``: the cross terms of |a - b|^2 on the matrix cores (split
    float16) rank the rows, the four best per query are re-evaluated exactly in float32 and
    an error bound proves the rest cannot beat them (else that query is rescanned exactly).
    ``scale``: ``_knn_scale`` of the largest magnitude of both sets when the caller knows it
    (no wait for the device's maximum).  That joint peak is also what is taken when ``scale`` is
    not given; the answer is guaranteed exact while ``des2``'s largest magnitude times the scale
    is at least 2^-3 (``pano_knn2``), i.e. while ``des2``'s peak is within 2^12 of the joint one:
    large ``des1`` against tiny ``des2`` falls outside the rule, and nothing reports it."""
    idx, dist, rescans = _knn2_raw(des1, des2, eng or _eng.engine(), scale)
    if want_rescans:
        return idx.long(), dist, int(rescans.item())
    return idx.long(), dist


def _knn2_raw(des1, des2, eng, scale=None):
    """``pano_knn2`` queued: (idx int32 [K1][2], dist float32 [K1][2], rescans int32 [1]) on the
    device."""
    import torch
    nq, d = (int(v) for v in des1.shape)
    nt = int(des2.shape[0])
    des1, des2 = des1.contiguous(), des2.contiguous()
    if scale is None:
        peak = float(torch.maximum(des1.abs().amax(), des2.abs().amax()).item()) if nq else 1.0
        scale = _knn_scale(peak)
    work = torch.empty(int(eng.lib.pano_knn2_work_bytes(nq, nt, d)), dtype=torch.uint8,
                       device=eng.device)
    idx = torch.empty((nq, 2), dtype=torch.int32, device=eng.device)
    dist = torch.empty((nq, 2), dtype=torch.float32, device=eng.device)
    rescans = torch.zeros(1, dtype=torch.int32, device=eng.device)
    eng.call("pano_knn2", des1, nq, des2, nt, d, scale, work, idx, dist, rescans)
    return idx, dist, rescans


def _ratio_test(dist, ratio):
    """Queries that pass Lowe's ratio test, ascending: float64(dist[q, 0]) < ratio *
    float64(dist[q, 1]), strict, as ``pano_match_pack`` compares and as the reference does on
    Python floats (features.py:232).  dist: float32 [K][2].  Compared in float32, as NumPy would
    on these arrays, ratio * dist[q, 1] is rounded once more and matches on the boundary are
    lost."""
    dist = np.asarray(dist).reshape(-1, 2).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.nonzero(dist[:, 0] < float(ratio) * dist[:, 1])[0]


def flann_matching(des1, des2, ratio=0.7):
    """Given 2 lists of descriptors, match them (features.py:222-232): 2-NN + Lowe's
    ratio test.  Exact search instead of FLANN's approximate one."""
    import torch
    eng = _eng.engine()
    if len(des1) == 0 or len(des2) < 2:
        return []
    d1 = torch.from_numpy(np.ascontiguousarray(des1, np.float32)).to(eng.device)
    d2 = torch.from_numpy(np.ascontiguousarray(des2, np.float32)).to(eng.device)
    idx, dist = knn2_device(d1, d2)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    keep = _ratio_test(dist, ratio)
    return [DMatch(q, idx[q, 0], dist[q, 0]) for q in keep]


# ------------------------------------------------------------- homographies (RANSAC)
RANSAC = 8                  # cv2.RANSAC
N_MIN_MATCH = 8             # features.py:17: minimum number of point matches
LOWE_RATIO = 0.7            # features.py:232


def find_homographies_device(pts, offsets, counts, max_iters=2000, thresh=3.0, seed=0,
                             want_scores=False, eng=None):
    """``pano_hom_ransac`` over a batch of pairs, device tensors in and out.
    pts: float32 [m][4] (src x, y, dst x, y; every pair's rows back to back), offsets / counts:
    int32 [n_pairs] (a pair with fewer than 4 rows fails).  Returns (hom float64 [n][3][3],
    h33 = 1, zeros where the pair failed; mask uint8 [m]; n_inliers int32 [n], 0 = failed),
    plus the scores int32 [n][max_iters] of every hypothesis (-1: invalid) with ``want_scores``.
    Queued on the current stream, nothing waited for."""
    import torch
    eng = eng or _eng.engine()
    dev = eng.device
    n = int(offsets.shape[0])
    pts = pts.reshape(-1, 4).to(device=dev, dtype=torch.float32).contiguous()
    offsets = offsets.to(device=dev, dtype=torch.int32).contiguous()
    counts = counts.to(device=dev, dtype=torch.int32).contiguous()
    max_iters = int(max_iters)
    if pts.shape[0] == 0:                   # (keeps the data pointer valid and aligned)
        pts = torch.zeros((1, 4), dtype=torch.float32, device=dev)
    hom = torch.zeros((n, 3, 3), dtype=torch.float64, device=dev)
    mask = torch.zeros(max(int(pts.shape[0]), 1), dtype=torch.uint8, device=dev)
    n_inl = torch.zeros(n, dtype=torch.int32, device=dev)
    scores = torch.empty((n, max_iters), dtype=torch.int32, device=dev) if want_scores else None
    work = None if want_scores else torch.empty(
        int(eng.lib.pano_hom_ransac_work_bytes(n, max_iters)), dtype=torch.uint8, device=dev)
    eng.call("pano_hom_ransac", pts, offsets, counts, n, max_iters, thresh,
             int(seed) & 0xFFFFFFFFFFFFFFFF, work, hom, mask, n_inl, scores)
    out = (hom, mask, n_inl)
    return out + (scores,) if want_scores else out


def find_homography(srcPoints, dstPoints, method=RANSAC, ransacReprojThreshold=3.0,
                    maxIters=2000, confidence=0.995, seed=0):
    """``cv2.findHomography(src, dst, cv2.RANSAC, ...)`` (features.py:244) on the GPU.
    Points (N, 2) or (N, 1, 2).  Returns (H float64 (3, 3) with H[2, 2] = 1, mask uint8 (N, 1)),
    or (None, None) when no homography is found.  Every one of ``maxIters`` hypotheses is scored:
    ``confidence`` is accepted for compatibility and not used; the refit is a normalised DLT over
    the inliers without OpenCV's Levenberg-Marquardt polish; ``seed`` picks the samples
    (include/pano360.h, pano_hom_ransac)."""
    import torch
    if method != RANSAC:
        raise ValueError(f"find_homography: method {method!r} (only RANSAC = {RANSAC})")
    src = np.asarray(srcPoints, np.float32).reshape(-1, 2)
    dst = np.asarray(dstPoints, np.float32).reshape(-1, 2)
    if len(src) != len(dst):
        raise ValueError(f"find_homography: {len(src)} source and {len(dst)} destination points")
    m = len(src)
    if m < 4:
        return None, None
    eng = _eng.engine()
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate([src, dst], axis=1))).to(eng.device)
    zero = torch.zeros(1, dtype=torch.int32)
    hom, mask, n_inl = find_homographies_device(pts, zero, torch.full((1,), m, dtype=torch.int32),
                                                maxIters, ransacReprojThreshold, seed, eng=eng)
    if int(n_inl.cpu()[0]) == 0:
        return None, None
    return hom[0].cpu().numpy(), mask[:m].cpu().numpy().reshape(m, 1)


class _Pairs:
    """Every pair's correspondences packed back to back on the device: per pair, the ratio test
    over ``pano_knn2`` (``pano_match_pack``) into a region of as many rows as the query image has
    keypoints, then ONE ``pano_hom_ransac`` over the pairs with at least N_MIN_MATCH survivors.
    Nothing is waited for until ``download``."""

    def __init__(self, kpts, descs, pairs, eng, max_iters=2000, thresh=3.0, seed=0):
        import torch
        self.pairs, dev = list(pairs), eng.device
        f32 = dict(dtype=torch.float32, device=dev)
        kp_dev = [torch.from_numpy(np.ascontiguousarray(k, np.float32).reshape(-1, 2)).to(dev)
                  for k in kpts]
        des_dev = [torch.from_numpy(np.ascontiguousarray(d, np.float32)).to(dev) for d in descs]
        peaks = [float(np.abs(d).max()) if len(d) else 0.0 for d in descs]
        sizes = [len(kpts[i]) for i, _ in self.pairs]
        self.offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        total = int(self.offsets[-1])
        self.pts = torch.zeros((max(total, 1), 4), **f32)
        self.match = torch.zeros((max(total, 1), 2), dtype=torch.int32, device=dev)
        self.counts = torch.zeros(len(self.pairs), dtype=torch.int32, device=dev)
        for p, (i, j) in enumerate(self.pairs):
            nq, nt = len(kpts[i]), len(kpts[j])
            if nq == 0 or nt < 2:
                continue
            idx, dist, _ = _knn2_raw(des_dev[i], des_dev[j], eng,
                                     _knn_scale(max(peaks[i], peaks[j])))
            off = int(self.offsets[p])
            eng.call("pano_match_pack", idx, dist, nq, LOWE_RATIO, kp_dev[i], kp_dev[j], nt,
                     self.pts[off:], self.match[off:], self.counts[p:])
        # pairs below N_MIN_MATCH survivors take part with no rows: they fail without a wait
        eff = torch.where(self.counts >= N_MIN_MATCH, self.counts, torch.zeros_like(self.counts))
        off_dev = torch.from_numpy(self.offsets[:-1].astype(np.int32)).to(dev)
        self.hom, self.mask, self.n_inl = find_homographies_device(
            self.pts, off_dev, eff, max_iters, thresh, seed, eng=eng)

    def download(self):
        """{(i, j): (match int32 [M][2] of the inliers, hom float64 (3, 3))} of the pairs that
        registered: one wait."""
        import torch
        host = [torch.empty(t.shape, dtype=t.dtype).pin_memory()
                for t in (self.counts, self.n_inl, self.hom, self.mask, self.match)]
        for h, t in zip(host, (self.counts, self.n_inl, self.hom, self.mask, self.match)):
            h.copy_(t, non_blocking=True)
        torch.cuda.current_stream(self.counts.device).synchronize()
        counts, n_inl, hom, mask, match = (h.numpy() for h in host)
        out = {}
        for p, pair in enumerate(self.pairs):
            if counts[p] < N_MIN_MATCH or n_inl[p] == 0:
                continue
            o, c = int(self.offsets[p]), int(counts[p])
            out[pair] = (match[o:o + c][mask[o:o + c] != 0].copy(), hom[p].copy())
        return out


def _match_hom(pt1, pt2, des1, des2):
    """Match points, estimate homography and return inlier matches (features.py:235-247):
    (match int32 [M][2] of the inliers, hom float64 (3, 3)), or (None, None) below N_MIN_MATCH
    ratio-test survivors or when RANSAC finds nothing."""
    got = _Pairs([pt1, pt2], [des1, des2], [(0, 1)], _eng.engine()).download()
    return got.get((0, 1), (None, None))


def _reverse(match, hom):
    """Find the matches and homography for the image is reverse order (features.py:250-252)."""
    return np.fliplr(match), np.linalg.inv(hom)


def _centred_keypoints(kp_, img):
    cent = np.array([img.shape[1], img.shape[0]]) / 2
    pts = np.array([kp.pt for kp in kp_], np.float64).reshape(-1, 2)
    return np.float32(pts - cent)


def matching(imgs, detect=sift_detector()):
    """Find correspondences between images in a list (features.py:255-283).
    Returns (kpts, matches): kpts a 1-D object array of N float32 [K_i][2] keypoint arrays,
    centred on the image; matches a 0-d object array holding a ``defaultdict(dict)`` with
    ``[i][j] = (int32 [M][2] inlier (query, train) indices, float64 (3, 3) homography i -> j)``
    and ``[j][i] = _reverse(...)``, inserted in the reference's loop order.  Every pair is
    matched on the device and all pairs share one RANSAC launch; a pair with fewer than
    N_MIN_MATCH ratio-test survivors, or whose RANSAC fails, gets no entry (the reference would
    stop on a failed findHomography)."""
    kpts, descs = [], []
    start = time.time()
    for i, img in enumerate(imgs):
        logging.debug(f"Processing image #{i+1}")
        kp_, des = detect(img)         # (host results: nothing of the detector's ring is held)
        kpts.append(_centred_keypoints(kp_, img))
        descs.append(np.asarray(des, np.float32).reshape(len(kp_), -1))
    logging.info(f"Extracted keypoints, time: {time.time() - start}")

    n_imgs = len(imgs)
    start = time.time()
    pairs = [(src, dst) for src in range(n_imgs) for dst in range(src + 1, n_imgs)]
    found = _Pairs(kpts, descs, pairs, _eng.engine()).download() if pairs else {}
    logging.info(f"Matched features, time: {time.time() - start}")
    return _assemble(kpts, found)


def _assemble(kpts, found):
    """matching's return value from the keypoints and {(src, dst): (match, hom)} of the pairs
    that registered: keys in the reference's loop order (src ascending, dst ascending, the
    reverse entry straight after), which is the order ``traverse`` walks them in."""
    matches, n_imgs = defaultdict(dict), len(kpts)
    for src in range(n_imgs):
        for dst in range(src + 1, n_imgs):
            if (src, dst) not in found:
                continue
            match, hom = found[(src, dst)]
            matches[src][dst] = (match, hom)
            matches[dst][src] = _reverse(match, hom)
    kpt_arr = np.empty(len(kpts), dtype=object)     # 1-D even when every K_i is the same
    for i, k in enumerate(kpts):
        kpt_arr[i] = k
    match_arr = np.empty((), dtype=object)
    match_arr[()] = matches
    return kpt_arr, match_arr


def parse_args(argv=None):
    """The command line of ``main``."""
    from . import fuse as _fuse
    from . import lens as _lens
    parser = argparse.ArgumentParser(description="Extract features.")
    parser.add_argument("--path", type=str, default="../data/ppwwyyxx/CMU2",
                        help="directory with the images to process.")
    parser.add_argument("--detector", default="sift", choices=["sift", "msop"],
                        help="feature detector (msop writes matches_<name>_msop.npz).")
    _lens.add_arguments(parser)
    _fuse.add_arguments(parser)
    args = parser.parse_args(argv)
    _lens.check_arguments(parser, args)
    _fuse.check_arguments(parser, args)
    return args


def cache_name(args):
    """``<name>`` of ``matches_<name>.npz``: the directory, ``_msop`` for that detector, ``_b<K>``
    with ``--bracket K`` (``_b<K>a`` with ``--bracket-align``, ``_b<K>g`` with ``--bracket-deghost``,
    ``_b<K>ag`` with both), ``_lens`` with ``--lens``."""
    from . import fuse as _fuse
    name = os.path.basename(args.path)
    if args.detector == "msop":
        name += "_msop"
    name += _fuse.cache_suffix(args)
    if args.lens is not None:
        name += "_lens"
    return name


def main(argv=None):
    """Script entry point (features.py:300-320): the images of ``--path``, shrunk by half,
    matched; writes ``matches_<name>.npz`` (``--detector msop``: ``matches_<name>_msop.npz``;
    ``--lens FILE``: the images' lens distortion corrected first, ``matches_<name>_lens.npz``;
    ``--bracket K``: every K files fused into one frame first, ``matches_<name>_b<K>.npz``).
    Read with Pillow, resized on the device."""
    from . import fuse as _fuse
    from . import lens as _lens
    from .stitcher import ingest
    args = parse_args(argv)
    name = cache_name(args)
    imgs = ingest(args.path, 2, lens=_lens.from_args(args), bracket=_fuse.from_args(args))
    kpts, matches = matching(imgs, **detector_kwargs(args.detector))
    np.savez(f"matches_{name}.npz", kpts=kpts, matches=matches)
    return kpts, matches


if __name__ == "__main__":
    logging.basicConfig(level=logging.DEBUG)
    main()
