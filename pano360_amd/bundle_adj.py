"""Cameras from pairwise matches: the camera record consumed by the warp/blend hot path and
the reference's registration stage (reference ``bundle_adj.py``).

``Image`` (``bundle_adj.py:18-33``), ``intrinsics`` (``:82-87``) and ``rotation_to_mat``
(``:96-101``) are the input type of the stitch.  The rest is the reference's bundle adjustment
with its semantics: focal estimation from a homography, the incremental walk over the best
pairs (``traverse``), Levenberg-Marquardt with a constant damping (``IncrementalBundleAdjuster``)
and straightening.  The per-match work of every LM iteration (residuals, the Jacobian of
``_jacobian_symbolic``, J^T J and J^T r) runs in ``csrc/bundle.hip`` in f64; the per-camera
3 x 3 algebra, the solve and the control flow stay here (include/pano360.h, pano_ba_normal).
``refine`` is not the reference's: a robust refinement of the cameras ``traverse`` made, with the
true derivative and optionally a shared radial distortion (``csrc/refine.hip``, pano_ba_refine).

The class is importable as ``bundle_adj.Image`` through the top-level
``bundle_adj.py`` re-export, so ``ba_<name>.pkl`` caches written by the
reference CLI (stitcher.py:430-439) unpickle into it unchanged.
"""
import heapq
import logging
from dataclasses import dataclass, field

import numpy as np

from . import _lib


def _zero_range():
    return (np.zeros(2), np.zeros(2))


class Deferred:
    """A pixel array that exists on the device and is copied to the host when first read
    (``stitch`` leaves the float32 RGBA image of ``_add_weights`` in ``reg.img``,
    stitcher.py:277-278: 133 MB per 4K frame that most callers never look at)."""

    def __init__(self, make):
        self.make = make


@dataclass(repr=False)
class Image:
    """One registered frame: pixels, rotation R, calibration K, angular range - a dataclass
    with the reference's four fields (``dataclasses.fields`` / ``asdict`` / ``replace`` and the
    keyword constructor work as they do on the reference's class).

    ``img``   uint8 [H, W, 3] on entry to ``stitch`` (channel order opaque); float32 RGBA
              afterwards, as in the reference.  ``stitch`` stores a ``Deferred`` there: the
              RGBA image is made on the device and downloaded when ``img`` is first READ.
              Until then the record keeps the device frame, the colour table and the engine
              alive; reading it (or assigning to it) releases them.  The read runs
              ``_add_weights`` on the engine's current stream at that moment.
    ``rot``   float64 3x3 world->camera rotation.
    ``intr``  float64 3x3 ``[[f,0,cx],[0,f,cy],[0,0,1]]``.
    ``range`` (min, max) spherical angles, filled in by ``stitch``.
    """

    img: np.ndarray
    rot: np.ndarray
    intr: np.ndarray
    range: tuple = field(default_factory=_zero_range)        # noqa: A003 - the reference's name

    # the reference's class pickles its plain attributes: keep that layout in both directions
    def __getstate__(self):
        return {"img": self.img, "rot": self.rot, "intr": self.intr, "range": self.range}

    def __setstate__(self, state):
        for key, value in state.items():
            setattr(self, key, value)

    def __repr__(self):
        return (f"Image(img={type(self.__dict__.get('_img')).__name__}, rot={self.rot!r}, "
                f"intr={self.intr!r}, range={self.range!r})")

    def hom(self):
        """Pixel -> ray: ``R^T K^-1`` (reference bundle_adj.py:27-29)."""
        return self.rot.T.dot(np.linalg.inv(self.intr))

    def proj(self):
        """Ray -> pixel: ``K R`` (reference bundle_adj.py:31-33)."""
        return self.intr.dot(self.rot)


def _img_get(self):
    value = self.__dict__.get("_img")
    if isinstance(value, Deferred):
        value = self.__dict__["_img"] = value.make()
    return value


def _img_set(self, value):
    self.__dict__["_img"] = value


# the field `img` is served by a property (attached after @dataclass has read the annotations):
# the generated __init__ / __eq__ / replace go through it like any other attribute access
Image.img = property(_img_get, _img_set)

# pickles name the class by module path: keep the reference's, so camera caches
# move between the reference CLI and this build in both directions
Image.__module__ = "bundle_adj"


def intrinsics(focal, center=(0, 0)):
    """Calibration matrix; like the reference (bundle_adj.py:82-87) a pair of
    focals is accepted but only the first one is used for both axes."""
    if not isinstance(focal, (list, tuple)):
        focal = (focal, focal)
    f = focal[0]
    return np.array([[f, 0, center[0]],
                     [0, f, center[1]],
                     [0, 0, 1]])


def rotation_to_mat(rad):
    """Rodrigues formula, exponential map -> matrix (bundle_adj.py:96-101).
    Unlike the reference there is no random default argument."""
    rad = np.asarray(rad, dtype=np.float64)
    ang = np.linalg.norm(rad)
    axis = rad / ang if ang else rad
    k = np.array([[0, -axis[2], axis[1]],
                  [axis[2], 0, -axis[0]],
                  [-axis[1], axis[0], 0]])
    return np.eye(3) + k * np.sin(ang) + (1 - np.cos(ang)) * k.dot(k)


# ------------------------------------------------------------------ constants (bundle_adj.py:8-15)
PARAMS_PER_CAMERA = 6       # f, ppx, ppy and the exponential map of the rotation
TERMS_PER_MATCH = 2         # residual x and y
LM_LAMBDA = 5               # constant Levenberg-Marquardt damping
LM_MAX_ITER = 100
MIN_MATCH_ERROR = 150       # a pair whose RMS error exceeds this when it joins is left out


# ------------------------------------------------------------------ focal from a homography
def _pick_focal(sq1, sq2, den1, den2):
    """Of two squared focal estimates, the one with the larger denominator when both are
    positive, else the positive one, else 0 (the values are ordered, the denominators are not)."""
    if sq1 < sq2:
        sq1, sq2 = sq2, sq1
    if sq1 > 0 and sq2 > 0:
        return np.sqrt(sq1 if abs(den1) > abs(den2) else sq2)
    if sq1 > 0:
        return np.sqrt(sq1)
    return 0


def _focal_of(hom):
    """Szeliski & Shum (1997): a rotation-only homography H = K1 R K0^-1 with principal points
    at the origin makes the rows (and the columns) of R orthonormal, which gives two estimates
    of f1^2 from H's third row and two of f0^2 from its first two rows; the result is the
    geometric mean of f0 and f1."""
    h = np.ravel(hom)
    with np.errstate(divide="ignore", invalid="ignore"):
        den1, den2 = h[6] * h[7], (h[7] - h[6]) * (h[7] + h[6])
        f1 = _pick_focal(-(h[0] * h[1] + h[3] * h[4]) / den1,
                         (h[0] * h[0] + h[3] * h[3] - h[1] * h[1] - h[4] * h[4]) / den2, den1, den2)
        den1 = h[0] * h[3] + h[1] * h[4]
        den2 = h[0] * h[0] + h[1] * h[1] - h[3] * h[3] - h[4] * h[4]
        f0 = _pick_focal(-h[2] * h[5] / den1, (h[5] * h[5] - h[2] * h[2]) / den2, den1, den2)
        return np.sqrt(f0 * f1)


def get_focal(hom):
    """Focal length from a homography (bundle_adj.py:69-79); the inverse homography is tried
    when the forward one gives no estimate."""
    focal = _focal_of(hom)
    return focal if focal else _focal_of(np.linalg.inv(hom))


# ------------------------------------------------------------------ rotations, stacked
def _skew(vec):
    """[..., 3] -> [..., 3, 3]: the matrix of the cross product with vec."""
    vec = np.asarray(vec, dtype=np.float64)
    out = np.zeros(vec.shape + (3,))
    out[..., 0, 1], out[..., 0, 2] = -vec[..., 2], vec[..., 1]
    out[..., 1, 0], out[..., 1, 2] = vec[..., 2], -vec[..., 0]
    out[..., 2, 0], out[..., 2, 1] = -vec[..., 1], vec[..., 0]
    return out


def _angles(rots):
    """[n, 3, 3] -> [n, 3]: the exponential map of each rotation (bundle_adj.py:104-115): the
    axis from the antisymmetric part, the angle from the trace; below 1e-7 of antisymmetric
    part, zero."""
    rots = np.asarray(rots, dtype=np.float64)
    rad = np.stack([rots[:, 2, 1] - rots[:, 1, 2], rots[:, 0, 2] - rots[:, 2, 0],
                    rots[:, 1, 0] - rots[:, 0, 1]], axis=1)
    mod = np.sqrt(np.sum(rad * rad, axis=1))
    small = mod < 1e-7
    trace = (rots[:, 0, 0] + rots[:, 1, 1]) + rots[:, 2, 2]
    theta = np.arccos(np.clip((trace - 1) / 2, -1, 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        rad = rad * (theta / mod)[:, None]
    rad[small] = 0.0
    return rad


def _rotations(rad):
    """[n, 3] -> [n, 3, 3]: Rodrigues' formula, as ``rotation_to_mat``."""
    rad = np.asarray(rad, dtype=np.float64)
    ang = np.sqrt(np.sum(rad * rad, axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        axis = np.where(ang[:, None] > 0, rad / ang[:, None], rad)
    k = _skew(axis)
    return (np.eye(3) + k * np.sin(ang)[:, None, None]
            + (1 - np.cos(ang))[:, None, None] * (k @ k))


def _dr_dvis(rots):
    """[n, 3, 3] -> [n, 3, 3, 3]: dR / dv_k of each rotation (bundle_adj.py:163-177), the
    derivative of the exponential map (Gallego & Yezzi 2015):
    dR/dv_k = (v_k [v]x + [v x (I - R) e_k]x) R / |v|^2, the generators [e_k]x near v = 0."""
    rots = np.asarray(rots, dtype=np.float64)
    rad = _angles(rots)
    vsqr = np.sum(np.square(rad), axis=1)
    ire = np.eye(3) - rots
    terms = _skew(rad)[:, None] * rad[:, :, None, None]
    terms = terms + _skew(np.cross(rad[:, None, :], np.swapaxes(ire, 1, 2)))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (terms @ rots[:, None]) / vsqr[:, None, None, None]
    out[vsqr < 1e-14] = _skew(np.eye(3))
    return out


def mat_to_angle(rot):
    """Exponential representation of a rotation matrix (bundle_adj.py:104-115)."""
    return _angles(np.asarray(rot)[None])[0]


def dr_dvi(rot):
    """The three derivatives of a rotation w.r.t. its exponential map (bundle_adj.py:163-177)."""
    return _dr_dvis(np.asarray(rot)[None])[0]


def to_rotation(rot):
    """The rotation nearest to ``rot`` in the Frobenius norm (U V^T of its SVD), with a
    reflection turned into a rotation by negation (bundle_adj.py:118-124)."""
    uu_, _, vv_ = np.linalg.svd(rot)
    rot = uu_.dot(vv_)
    if np.linalg.det(rot) < 0:
        rot = -rot
    return rot


# ------------------------------------------------------------------ cameras and residuals
def params_to_camera(params):
    """(f, ppx, ppy, v0, v1, v2) -> a camera without pixels (bundle_adj.py:131-135)."""
    foc, x_c, y_c = params[:3]
    return Image(None, rotation_to_mat(params[3:]), intrinsics(foc, (x_c, y_c)))


def camera_to_params(camera):
    """A camera -> (f, ppx, ppy, v0, v1, v2) (bundle_adj.py:138-142)."""
    intr = camera.intr
    return np.concatenate([[intr[0, 0], intr[0, 2], intr[1, 2]], mat_to_angle(camera.rot)])


def _hom(cam_b, cam_a):
    """K_b R_b R_a^T K_a^-1: pixels of camera a to pixels of camera b (bundle_adj.py:36-38)."""
    return cam_b.intr.dot(cam_b.rot).dot(cam_a.rot.T.dot(np.linalg.inv(cam_a.intr)))


def get_diff(cam1, cam2, match):
    """Residuals of one pair's matches, all x then all y (bundle_adj.py:145-149): columns
    0..2 of ``match`` seen by cam1, 3..5 by cam2."""
    proj = _hom(cam1, cam2).dot(match[:, 3:6].T)
    return (match[:, :3].T - proj / proj[[-1], :])[:-1].ravel()


def residuals(cameras, matches):
    """Every pair's residuals back to back (bundle_adj.py:152-155)."""
    return np.concatenate([get_diff(cameras[b], cameras[a], m) for a, b, m in matches], axis=0)


def loss(res):
    """Root mean square of the residuals (bundle_adj.py:158-160)."""
    return np.sqrt(np.mean(np.square(res)))


def straighten(rots):
    """A global rotation that levels the panorama (bundle_adj.py:398-414): the cameras' x axes
    are taken to lie in one plane, whose normal (the smallest principal axis of their
    covariance) becomes the up axis; the cameras' mean viewing direction fixes the rest."""
    cov = np.cov(np.stack([rot[0] for rot in rots], axis=-1))
    v_y = np.linalg.svd(cov)[2][2]
    v_z = np.sum(np.stack([rot[2] for rot in rots], axis=0), axis=0)
    v_x = np.cross(v_y, v_z)
    v_x /= np.linalg.norm(v_x)
    v_z = np.cross(v_x, v_y)
    if np.sum([v_x.dot(rot[0]) for rot in rots]) < 0:
        v_x, v_y = -v_x, -v_y
    glob = np.stack([v_x, v_y, v_z], axis=-1)
    return [rot.dot(glob) for rot in rots]


# ------------------------------------------------------------------ the device side
def _pair_homs(K, R, Kinv, a, b):
    """[p, 3, 3]: K_b R_b R_a^T K_a^-1 for the pairs (a[p], b[p]) of one camera state."""
    return (K[b] @ R[b]) @ (np.swapaxes(R[a], 1, 2) @ Kinv[a])


def _jacobian_tables(K, R, Kinv, dR, a, b):
    """[p, 90]: the ten 3 x 3 tables per pair of pano_ba_normal (include/pano360.h), at one
    camera state."""
    Rt_a = np.swapaxes(R[a], 1, 2)
    KR_b = K[b] @ R[b]
    hom = KR_b @ (Rt_a @ Kinv[a])
    s_b = (R[b] @ Rt_a) @ Kinv[a]
    s_r = Rt_a @ Kinv[a]
    n_k = K[b][:, None] @ dR[b]
    q_k = KR_b[:, None] @ np.swapaxes(dR[a], 2, 3)
    tabs = np.concatenate([hom[:, None], s_b[:, None], s_r[:, None], Kinv[a][:, None], n_k, q_k],
                          axis=1)
    return np.ascontiguousarray(tabs.reshape(len(a), 90))


class _State:
    """One set of cameras as stacked arrays over every camera index (identity where inactive)."""

    def __init__(self, K, R):
        self.K, self.R = K, R
        self.Kinv = np.linalg.inv(K)

    @classmethod
    def of(cls, cameras):
        eye = np.eye(3)
        return cls(np.stack([eye if c is None else c.intr for c in cameras]).astype(np.float64),
                   np.stack([eye if c is None else c.rot for c in cameras]).astype(np.float64))


class _Device:
    """The matches of one adjuster on the device, and the buffers of its LM iterations.
    Rows are appended as pairs are considered and stay for the adjuster's life."""

    def __init__(self, n_cameras):
        import torch
        from . import engine as _eng
        self.torch, self.eng = torch, _eng.engine()
        self.dev = self.eng.device
        self.rows = torch.zeros((1024, 4), dtype=torch.float64, device=self.dev)
        self.n_rows = 0
        self.n_cameras = n_cameras

    def append(self, rows):
        """Upload [k][4] rows; returns their first row index."""
        torch = self.torch
        need = self.n_rows + len(rows)
        if need > self.rows.shape[0]:
            grown = torch.zeros((max(need, 2 * self.rows.shape[0]), 4), dtype=torch.float64,
                                device=self.dev)
            grown[:self.n_rows] = self.rows[:self.n_rows]
            self.rows = grown
        first = self.n_rows
        if len(rows):
            self.rows[first:need] = torch.from_numpy(np.ascontiguousarray(rows)).to(self.dev)
        self.n_rows = need
        return first

    def upload(self, arr, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(arr, dtype=dtype)).to(self.dev)

    def download(self, *tensors):
        """Host copies of device tensors after one wait on the current stream."""
        torch = self.torch
        host = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in tensors]
        for h, t in zip(host, tensors):
            h.copy_(t, non_blocking=True)
        torch.cuda.current_stream(self.dev).synchronize()
        return [h.numpy() for h in host]

    def pair_ssq(self, pairs_dev, n_pairs, homs):
        """Per-pair sums of squared residuals (pano_ba_residuals), on the device."""
        hom = self.upload(homs.reshape(n_pairs, 9), np.float64)
        ssq = self.torch.empty(n_pairs, dtype=self.torch.float64, device=self.dev)
        self.eng.call("pano_ba_residuals", self.rows, pairs_dev, n_pairs, hom, ssq)
        return ssq

    def normal(self, pairs_dev, n_pairs, slot_dev, n_active, jtab, hom_r, work):
        """(J^T J + LM_LAMBDA I, J^T r) on the device (pano_ba_normal)."""
        torch = self.torch
        tab = self.upload(np.concatenate([jtab.reshape(-1), hom_r.reshape(-1)]), np.float64)
        n = PARAMS_PER_CAMERA * n_active
        jtj = torch.empty((n, n), dtype=torch.float64, device=self.dev)
        jtr = torch.empty(n, dtype=torch.float64, device=self.dev)
        self.eng.call("pano_ba_normal", self.rows, pairs_dev, n_pairs, slot_dev, n_active, tab,
                      tab.data_ptr() + 8 * 90 * n_pairs, LM_LAMBDA, work, jtj, jtr)
        return jtj, jtr


def _rms(ssq, counts):
    """loss over pairs from their sums of squares: sqrt(sum / (2 matches))."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(np.sum(ssq) / (TERMS_PER_MATCH * np.sum(counts)))


class IncrementalBundleAdjuster:
    """Bundle adjustment one camera at a time (bundle_adj.py:288-345).  ``cameras`` and
    ``matches`` ((a, b, rows) with rows [M][6] seen by b then a) are the reference's.
    ``history`` holds one record per ``optimize`` call: the initial loss, every candidate's
    loss and whether it was accepted."""

    def __init__(self, n_cameras, mode="incr"):
        self.cameras = [None] * n_cameras
        self.matches = []
        self.mode = mode
        self.history = []
        self._dev = None
        self._first = []            # first device row of each entry of self.matches

    def _device(self):
        if self._dev is None:
            self._dev = _Device(len(self.cameras))
        while len(self._first) < len(self.matches):      # pairs appended from outside
            self._first.append(self._dev.append(_rows_of(self.matches[len(self._first)][2])))
        return self._dev

    def _pair_table(self, a, b, first, counts):
        return self._dev.upload(np.stack([a, b, first, counts], axis=1), np.int32)

    def add(self, idx, camera, matches):
        """Add a camera and its pairs with the cameras already present; a pair whose RMS error
        at the current cameras exceeds MIN_MATCH_ERROR is left out (bundle_adj.py:297-309)."""
        dev = self._device()
        self.cameras[idx] = camera
        cands = [(new, matches[idx][new][0]) for new, cam in enumerate(self.cameras)
                 if cam is not None and new in matches[idx]]
        if cands:
            first = np.array([dev.append(_rows_of(m)) for _, m in cands], np.int64)
            counts = np.array([len(m) for _, m in cands], np.int64)
            a = np.array([new for new, _ in cands], np.int64)
            b = np.full(len(cands), idx, np.int64)
            state = _State.of(self.cameras)
            ssq = dev.download(dev.pair_ssq(self._pair_table(a, b, first, counts), len(cands),
                                            _pair_homs(state.K, state.R, state.Kinv, a, b)))[0]
            for k, (new, match) in enumerate(cands):
                if _rms(ssq[k:k + 1], counts[k:k + 1]) > MIN_MATCH_ERROR:
                    continue
                self.matches.append((new, idx, match))
                self._first.append(int(first[k]))
        if self.mode == "incr":
            self.optimize()

    def optimize(self):
        """Levenberg-Marquardt over the present cameras (bundle_adj.py:311-345): a constant
        damping LM_LAMBDA, a step kept only if it lowers the loss by more than 1e-3, a stop
        after the sixth step that is not kept (the count never resets) or LM_MAX_ITER steps.
        J^T J and J^T r are built on the device; the solve is NumPy's.  J^T r pairs J at the
        kept cameras with the residual of the last candidate, kept or not, as the reference's
        ``errs`` does."""
        if not self.matches:
            raise ValueError("optimize: no pairs between the cameras")
        dev = self._device()
        idx = np.array([i for i, c in enumerate(self.cameras) if c is not None], np.int64)
        a = np.array([m[0] for m in self.matches], np.int64)
        b = np.array([m[1] for m in self.matches], np.int64)
        counts = np.array([len(m[2]) for m in self.matches], np.int64)
        n_pairs = len(a)
        pairs = self._pair_table(a, b, np.array(self._first, np.int64), counts)
        slot = np.full(len(self.cameras), -1, np.int64)
        slot[idx] = np.arange(len(idx))
        slot = dev.upload(slot, np.int32)
        work = dev.torch.empty(int(dev.eng.lib.pano_ba_work_bytes(n_pairs)), dtype=dev.torch.uint8,
                               device=dev.dev)

        state = _State.of(self.cameras)
        hom_r = _pair_homs(state.K, state.R, state.Kinv, a, b)
        best = _rms(dev.download(dev.pair_ssq(pairs, n_pairs, hom_r))[0], counts)
        record = {"initial": float(best), "losses": [], "accepted": []}
        self.history.append(record)
        logging.debug(f"Optimizing {len(idx)} cameras, initial error: {best}")

        jtab, changed, n_not_improved = None, False, 0
        for _ in range(LM_MAX_ITER):
            if jtab is None:            # the tables change only when a step is kept
                jtab = _jacobian_tables(state.K, state.R, state.Kinv, _dr_dvis(state.R), a, b)
            jtj, jtr = dev.download(*dev.normal(pairs, n_pairs, slot, len(idx), jtab, hom_r,
                                                work))
            params = np.concatenate([np.stack([state.K[idx, 0, 0], state.K[idx, 0, 2],
                                               state.K[idx, 1, 2]], axis=1),
                                     _angles(state.R[idx])], axis=1)
            params -= np.linalg.solve(jtj, jtr).reshape(params.shape)

            K, R = state.K.copy(), state.R.copy()
            K[idx] = 0.0
            K[idx, 0, 0] = K[idx, 1, 1] = params[:, 0]
            K[idx, 0, 2], K[idx, 1, 2], K[idx, 2, 2] = params[:, 1], params[:, 2], 1.0
            R[idx] = _rotations(params[:, 3:])
            cand = _State(K, R)
            hom_r = _pair_homs(cand.K, cand.R, cand.Kinv, a, b)
            err = _rms(dev.download(dev.pair_ssq(pairs, n_pairs, hom_r))[0], counts)
            keep = bool(err < best - 1e-3)
            record["losses"].append(float(err))
            record["accepted"].append(keep)
            if keep:
                best, state, jtab, changed = err, cand, None, True
            else:
                n_not_improved += 1
                if n_not_improved > 5:
                    break
        logging.debug(f"Final error: {best} after {len(record['losses'])} iterations")
        if changed:
            cams = list(self.cameras)
            for i in idx:
                cams[i] = Image(None, state.R[i].copy(), state.K[i].copy())
            self.cameras = cams


def _rows_of(match):
    """Device rows (x_b, y_b, x_a, y_a) of the reference's [M][6] homogeneous match rows."""
    match = np.asarray(match, dtype=np.float64).reshape(-1, 6)
    return match[:, [0, 1, 3, 4]]


def traverse(imgs, matches, badjust="incr", use_straighten=True):
    """Cameras from pairwise matches (bundle_adj.py:348-395).  ``matches[i][j]`` is
    (rows [M][6], homography i <- j, number of inliers), as ``stitcher.idx_to_keypoints``
    makes it.  The pair with the most inliers starts the walk at the identity with the median
    of the homographies' focal estimates; every camera then joins through its best pair with
    a placed camera, rotation from that pair's homography.  ``badjust``: "incr" optimizes after
    every camera, "last" once at the end, "none" never.  Returns the cameras that were
    reached, in index order, with ``imgs[i]`` attached (host arrays or device frames alike)."""
    entries = [(i, matches[i][j][1], matches[i][j][2]) for i in matches for j in matches[i]]
    if not entries:
        raise ValueError("traverse: no pairs")
    src = entries[int(np.argmax([e[2] for e in entries]))][0]
    intr = intrinsics(np.median([get_focal(e[1]) for e in entries]))

    iba = IncrementalBundleAdjuster(len(imgs), mode=badjust)
    iba.cameras[src] = Image(None, np.eye(3), intr)
    queue = [(-matches[src][j][2], src, j) for j in matches[src]]
    heapq.heapify(queue)
    while queue:
        _, src, dst = heapq.heappop(queue)
        if iba.cameras[dst] is not None:
            continue
        rot = to_rotation(np.linalg.inv(intr).dot(matches[src][dst][1].dot(intr)))
        iba.add(dst, Image(None, rot.dot(iba.cameras[src].rot), intr), matches)
        for new in matches[dst]:
            heapq.heappush(queue, (-matches[dst][new][2], dst, new))
    if badjust == "last":
        iba.optimize()

    cameras = iba.cameras
    for i, img in enumerate(imgs):
        if cameras[i] is not None:
            cameras[i].img = img
    cameras = [c for c in cameras if c is not None]
    if use_straighten:
        for cam, rot in zip(cameras, straighten([c.rot for c in cameras])):
            cam.rot = rot
    return cameras


# ------------------------------------------------------------------ robust refinement
REFINE_TERMS = _lib.BA_REFINE_TERMS     # pano_ba_refine's sums per pair
REFINE_LOCAL = 10           # a pair's local parameters: f_b, omega_b, f_a, omega_a, k1, k2
REFINE_LAMBDA = 1e-3        # the first damping; / 10 after a step that is taken, * 10 otherwise
REFINE_LAMBDA_MAX = 1e12
REFINE_MIN_DECREASE = 1e-10


@dataclass
class Refinement:
    """What ``refine`` returns.  ``cameras``: new ``Image`` records (``img`` carried over);
    ``k``: (k1, k2); ``history``: one (cost, lambda, accepted) per iteration, cost the candidate's
    sum of Huber losses; ``rms_before`` / ``rms_after``: the root of the mean squared distance
    (pixels, per match) over the matches within the Huber threshold, at the cameras given and at
    the cameras returned; ``inlier_share``: those matches' share of all matches, and
    ``n_invalid`` the matches without a residual, both at the cameras returned."""
    cameras: list
    k: tuple
    history: list
    rms_before: float
    rms_after: float
    inlier_share: float
    n_invalid: int

    def lens_models(self, sizes):
        """One ``lens.LensModel`` per camera for ``lens.undistort_device``: the forward Brown
        model of the fitted (k1, k2) at the camera's focal length and principal point.
        ``sizes``: one (w, h), or one per camera."""
        from . import lens as _lens
        if len(sizes) == 2 and np.ndim(sizes[0]) == 0:
            sizes = [sizes] * len(self.cameras)
        if len(sizes) != len(self.cameras):
            raise ValueError(f"{len(sizes)} sizes for {len(self.cameras)} cameras")
        return [_lens.LensModel("brown", fx=cam.intr[0, 0], fy=cam.intr[0, 0],
                                cx=w / 2 + cam.intr[0, 2], cy=h / 2 + cam.intr[1, 2],
                                k=self.k, size=(w, h))
                for cam, (w, h) in zip(self.cameras, sizes)]


def _refine_pairs(matches, index):
    """[(a, b, rows [M][4])]: every unordered pair of ``matches`` between two images of ``index``
    once, in ascending (i, j), i < j: camera b is i's position, camera a is j's."""
    slot = {int(img): k for k, img in enumerate(index)}
    out = []
    keys = sorted({(min(i, j), max(i, j)) for i in matches for j in matches[i] if i != j})
    for i, j in keys:
        if i not in slot or j not in slot:
            continue
        if i in matches and j in matches[i]:
            rows = _rows_of(matches[i][j][0])
        else:
            rows = _rows_of(matches[j][i][0])[:, [2, 3, 0, 1]]
        out.append((slot[j], slot[i], rows))
    return out


def _refine_map(n, pairs, lens_terms, shared_focal):
    """[4 n + 2] -> the reduced system's index of every full parameter (camera c: f, omega at
    4 c .. 4 c + 3; k1, k2 last), -1 where it is not estimated: the rotation of the first camera
    that has a match (the gauge), the cameras without a pair, the k beyond ``lens_terms``; with
    ``shared_focal`` every f is the one parameter 0."""
    used = np.zeros(n, bool)
    for a, b, rows in pairs:
        if len(rows):
            used[a] = used[b] = True
    red = np.full(4 * n + 2, -1, np.int64)
    nxt = 1 if shared_focal else 0
    gauge = int(np.argmax(used))
    for c in range(n):
        if not used[c]:
            continue
        if shared_focal:
            red[4 * c] = 0
        else:
            red[4 * c], nxt = nxt, nxt + 1
        if c != gauge:
            red[4 * c + 1:4 * c + 4] = np.arange(nxt, nxt + 3)
            nxt += 3
    for t in range(lens_terms):
        red[4 * n + t], nxt = nxt, nxt + 1
    return red, nxt


class _Refiner:
    """The matches of one ``refine`` on the device and its evaluations: one pano_ba_refine and
    one wait each."""

    def __init__(self, pairs, n, huber):
        self.dev = _Device(n)
        self.n, self.huber = n, float(huber)
        firsts = [self.dev.append(rows) for _, _, rows in pairs]
        table = np.array([(a, b, first, len(rows)) for (a, b, rows), first in zip(pairs, firsts)],
                         np.int64).reshape(-1, 4)
        self.n_pairs = len(table)
        self.pairs = self.dev.upload(table, np.int32)
        self.out = self.dev.torch.empty((self.n_pairs, REFINE_TERMS),
                                        dtype=self.dev.torch.float64, device=self.dev.dev)

    def sums(self, f, pp, R, k):
        """out [n_pairs][70] at one state."""
        dev = self.dev
        cams = dev.upload(np.concatenate([f[:, None], pp, R.reshape(self.n, 9)], axis=1),
                          np.float64)
        dev.eng.call("pano_ba_refine", dev.rows, dev.n_rows, self.pairs, self.n_pairs, cams, self.n,
                     k[0], k[1], self.huber, self.out)
        return dev.download(self.out)[0].copy()


def _centre(focal, pp):
    """The least rotation C that takes the ray of the principal point ``pp`` of a camera that
    looks along z, (-px / f, -py / f, 1), to z: C R with the principal point at the centre looks
    where R with ``pp`` looked."""
    ray = np.array([-pp[0] / focal, -pp[1] / focal, 1.0])
    ray /= np.linalg.norm(ray)
    axis = np.cross(ray, [0.0, 0.0, 1.0])
    sin = np.linalg.norm(axis)
    return rotation_to_mat(axis / sin * np.arctan2(sin, ray[2])) if sin > 0 else np.eye(3)


def _refine_where(pairs, n):
    """[n_pairs][10]: where a pair's local parameters (f_b, omega_b, f_a, omega_a, k1, k2) are
    among the 4 n + 2."""
    a = np.array([p[0] for p in pairs], np.int64)
    b = np.array([p[1] for p in pairs], np.int64)
    return np.concatenate([4 * b[:, None] + np.arange(4), 4 * a[:, None] + np.arange(4),
                           np.tile([4 * n, 4 * n + 1], (len(pairs), 1))], axis=1)


def _refine_system(out, where, red, size):
    """(A, g) of the reduced system from the per-pair blocks, the pairs added in order."""
    uu, vv = np.triu_indices(REFINE_LOCAL)
    A, g = np.zeros((size, size)), np.zeros(size)
    ru, rv = red[where[:, uu]], red[where[:, vv]]
    val = out[:, :55]
    keep = (ru >= 0) & (rv >= 0)
    np.add.at(A, (ru[keep], rv[keep]), val[keep])
    keep &= (uu != vv)[None, :]
    np.add.at(A, (rv[keep], ru[keep]), val[keep])
    rg = red[where]
    keep = rg >= 0
    np.add.at(g, rg[keep], out[:, 55:65][keep])
    return A, g


def _refine_totals(out):
    """(cost, invalid, sum n^2 of the inliers, inliers) of one evaluation, the pairs in order."""
    cost = ssq = 0.0
    for row in out:
        cost, ssq = cost + row[65], ssq + row[68]
    return cost, int(round(np.sum(out[:, 67]))), ssq, int(round(np.sum(out[:, 69])))


def refine(cameras, matches, index=None, *, lens_terms=0, shared_focal=None, huber=3.0,
           max_iter=100):
    """A robust refinement of registered cameras, optionally with a radial distortion shared by
    all of them: the stage after ``traverse``, which stays the reference's step for step.

    ``cameras``: ``Image`` records as ``traverse`` returns them; ``matches``: the dict
    ``traverse`` takes; ``index[k]``: the image number of ``cameras[k]`` (None: camera k is image
    k; ``ValueError`` when the lengths make that impossible).  Every unordered pair of
    ``matches`` between two images present is used once, the pairs ``traverse``'s gate dropped
    included: the Huber loss deals with them.  ``huber`` is its threshold in pixels; 3.0 is the
    project's RANSAC threshold (``features.find_homographies_device``, ``thresh=3.0``): what the
    matcher calls an inlier is what the refinement weighs in full.  ``lens_terms``: 0, 1 (k1) or
    2 (k1 and k2) of ``r (1 + k1 r^2 + k2 r^4) = r_d`` in units of the focal length;
    ``shared_focal`` (default: ``lens_terms > 0``, since k is expressed in units of f and a focal
    length per camera leaves it weakly determined) gives all cameras one focal length.

    The distortion is centred on the principal point and everything behind the registration
    takes that for the image centre, while ``traverse`` moves it freely (by hundreds of pixels on
    noisy rings): each camera's principal point is therefore first folded into its rotation
    (``_centre``) and the cameras returned have it at the centre; with ``shared_focal`` the focal
    lengths start at their median.  Then Levenberg-Marquardt in float64 on the host over f (one
    per camera, or the one shared), the rotations (that of the first camera with a match is the
    gauge and stays: ``traverse``'s straightening survives) and k.  The per-match work (the
    residual under the distortion, its true derivative, the Huber weights, the per-pair sums) is
    pano_ba_refine (include/pano360.h): one call and one wait per iteration, since the call that scores a
    candidate holds the system of the next step.  ``(A + lambda diag A) step = -g`` from lambda
    = 1e-3; a candidate is taken when the sum of losses falls (and no further match lost its
    residual), lambda / 10, else lambda * 10; the loop ends after a taken step's relative
    decrease below 1e-10, with lambda above 1e12, or after ``max_iter`` iterations.
    Returns a ``Refinement``; the input records are not modified."""
    cameras = list(cameras)
    n = len(cameras)
    if lens_terms not in (0, 1, 2):
        raise ValueError(f"lens_terms={lens_terms!r}: 0, 1 or 2")
    if not (np.isfinite(huber) and huber > 0):
        raise ValueError(f"huber={huber!r}: a positive number of pixels")
    if index is None:
        images = {int(i) for i in matches} | {int(j) for i in matches for j in matches[i]}
        if n == 0 or (images and max(images) >= n):
            raise ValueError(f"{n} cameras for matches between images up to "
                             f"{max(images) if images else 0}: pass index")
        index = range(n)
    index = [int(i) for i in index]
    if len(index) != n or len(set(index)) != n:
        raise ValueError(f"index: {len(index)} image numbers ({len(set(index))} distinct) for "
                         f"{n} cameras")
    if shared_focal is None:
        shared_focal = lens_terms > 0
    pairs = _refine_pairs(matches, index)
    if not any(len(rows) for _, _, rows in pairs):
        raise ValueError("refine: no matches between the cameras")

    f = np.array([c.intr[0, 0] for c in cameras], np.float64)
    pp = np.array([[c.intr[0, 2], c.intr[1, 2]] for c in cameras], np.float64)
    R = np.stack([np.asarray(c.rot, np.float64) for c in cameras])
    R, pp = np.stack([_centre(f[c], pp[c]).dot(R[c]) for c in range(n)]), np.zeros((n, 2))
    if shared_focal:
        f = np.full(n, np.median(f))
    k = np.zeros(2)
    red, size = _refine_map(n, pairs, lens_terms, bool(shared_focal))
    dev = _Refiner(pairs, n, huber)
    where = _refine_where(pairs, n)
    n_matches = sum(len(rows) for _, _, rows in pairs)

    cur = dev.sums(f, pp, R, k)
    cost, invalid, ssq, inl = _refine_totals(cur)
    rms_before = float(np.sqrt(ssq / inl)) if inl else float("nan")
    history, lam = [], REFINE_LAMBDA
    for _ in range(max_iter):
        if lam > REFINE_LAMBDA_MAX:
            break
        A, g = _refine_system(cur, where, red, size)
        try:
            step = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
        except np.linalg.LinAlgError:
            step = None
        if step is None or not np.all(np.isfinite(step)):
            history.append((float("nan"), lam, False))
            lam *= 10
            continue
        full = np.where(red >= 0, step[np.maximum(red, 0)], 0.0)
        f_c = f + full[0:4 * n:4]
        R_c = np.stack([rotation_to_mat(full[4 * c + 1:4 * c + 4]).dot(R[c]) for c in range(n)])
        k_c = k + full[4 * n:]
        cand = dev.sums(f_c, pp, R_c, k_c)
        c_cost, c_invalid, c_ssq, c_inl = _refine_totals(cand)
        keep = bool(c_cost < cost and c_invalid <= invalid)
        history.append((float(c_cost), lam, keep))
        if keep:
            decrease = (cost - c_cost) / cost
            f, R, k, cur = f_c, R_c, k_c, cand
            cost, invalid, ssq, inl = c_cost, c_invalid, c_ssq, c_inl
            lam /= 10
            if decrease < REFINE_MIN_DECREASE:
                break
        else:
            lam *= 10
    # (a Deferred image is handed on as it is, not downloaded)
    out = [Image(c.__dict__.get("_img"), R[i].copy(),
                 intrinsics(float(f[i]), (float(pp[i, 0]), float(pp[i, 1]))), c.range)
           for i, c in enumerate(cameras)]
    return Refinement(out, (float(k[0]), float(k[1])), history, rms_before,
                      float(np.sqrt(ssq / inl)) if inl else float("nan"),
                      inl / n_matches, invalid)
