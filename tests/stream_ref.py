"""Reference of the streaming RGB-D Frame constructor (coeb_rgbd_stream_frame, src/Frame.cc:157-223):
the oracle's pieces composed frame by frame -- process_moving_object(frame f-1, frame f), blur_flags
of frame f's boxes, Extractor.extract with both, undistort_keypoints, and stereo_from_rgbd at the
RAW keypoint with uRight formed from the UNDISTORTED x (:829-839).  A frame without predecessor
takes the first-frame rule (:205-209: no T_M, every flag 0); process_moving_object returning None
(findFundamentalMat gave an empty matrix) is n_tm = -1 and an extraction without T_M.

The sequences are synth.moving_object_sequence scenes; everything is computed once per process
and handed out read-only."""
import functools

import numpy as np

import oracle as O
from coeb_front import KEYPOINT_DTYPE, synth

# TUM1 (freiburg1) calibration, as tests/test_gpu_frame_rgbd.py
FX, FY, CX, CY = 517.306408, 516.469215, 318.643040, 255.313989
TUM1 = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)
BF = synth.TUM_BF
U16_SCALE = 1.0 / 5000.0        # TUM DepthMapFactor 5000

# name -> size, frames, the object (x, y, w, h) and its step, and the second, static box.  The VGA
# sequence and its boxes are those of test_frame_batch_matches_oracle_frame_by_frame; the small ones
# scale its object so that it stays inside the frame.  The static box of "small" lies on a smooth
# stretch of the canvas (its Laplacian mean stays below 4.2: flag 1), the others on a textured
# panel (flag 0).  orb: the ORBextractor parameters; a 160 x 120 frame is too small for eight
# levels (the oracle and the plan both refuse it), so "small" runs with two.
ORB_DEFAULT = (1000, 1.2, 8, 20, 7)
SEQUENCES = {
    "vga": dict(w=640, h=480, n=6, seed=3, obj=(200, 120, 160, 200), shift=(-5, 4), static=(420, 60, 600, 200),
                orb=ORB_DEFAULT),
    "odd": dict(w=333, h=251, n=5, seed=3, obj=(104, 62, 83, 104), shift=(-3, 2), static=(218, 31, 312, 104),
                orb=ORB_DEFAULT),
    "small": dict(w=160, h=120, n=5, seed=3, obj=(60, 20, 48, 60), shift=(-4, 3), static=(60, 96, 84, 114),
                  orb=(1000, 1.2, 2, 20, 7)),
}


def camera_params(w, h):
    """TUM1 intrinsics scaled to a w x h frame (the distortion coefficients are size-free)."""
    sx, sy = w / 640.0, h / 480.0
    return FX * sx, FY * sy, CX * sx, CY * sy


def depth_map(w, h, kind="f32"):
    """Every pixel its own value with one hole of each class `d > 0` rejects: 0, negative, NaN
    ("f32"); "u16": the same surface in 1/5000 m with a zero hole (the only one 16U can hold)."""
    yy, xx = np.mgrid[0:h, 0:w]
    d = (1 + 0.001 * xx + 0.0007 * yy).astype(np.float32)
    d[h // 12:h * 5 // 12, w // 21:w * 25 // 64] = 0
    if kind == "u16":
        return np.round(d * 5000).astype(np.uint16)
    d[h * 11 // 24:h * 11 // 16, w * 33 // 64:w * 13 // 16] = -1.5
    d[h * 5 // 8:h * 7 // 8, w // 16:w * 5 // 16] = np.nan
    return d


def depth_float(depth):
    """imDepth as GrabImageRGBD hands it to the Frame: convertTo(CV_32F, scale) of a 16U map."""
    if depth.dtype == np.uint16:
        return depth.astype(np.float32) * np.float32(U16_SCALE)
    return np.ascontiguousarray(depth, np.float32)


@functools.lru_cache(maxsize=None)
def sequence(name):
    s = SEQUENCES[name]
    frames, obj = synth.moving_object_sequence(s["w"], s["h"], s["n"], seed=s["seed"], obj=s["obj"], obj_shift=s["shift"])
    boxes = [np.stack([obj[f], np.float32(s["static"])]) for f in range(s["n"])]
    frames.setflags(write=False)
    return frames, boxes


@functools.lru_cache(maxsize=None)
def extractor(orb=ORB_DEFAULT):
    return O.Extractor(*orb)


_tm_cache = {}


def moving_points(prev, cur):
    """process_moving_object, remembered per pair of frames"""
    key = (prev.shape, hash(prev.tobytes()), hash(cur.tobytes()))
    if key not in _tm_cache:
        _tm_cache[key] = O.process_moving_object(np.ascontiguousarray(prev), np.ascontiguousarray(cur))
    return _tm_cache[key]


def frame_ref(prev, cur, boxes, depth, dist=TUM1, orb=ORB_DEFAULT):
    """Frame.cc:157-223 for one frame: prev = imGrayPre or None (a first frame).  Returns
    dict(tm, n_tm, blur, kps, kps_un, desc, u_right, depth, first)."""
    h, w = cur.shape
    nbox = 0 if boxes is None else len(boxes)
    if prev is None:
        tm, n_tm, blur = None, 0, np.zeros(nbox, np.int32)
    else:
        tm = moving_points(prev, cur)
        n_tm = -1 if tm is None else len(tm)
        blur = O.blur_flags(cur, boxes)[0].astype(np.int32) if nbox else np.zeros(0, np.int32)
    tm_used = np.zeros((0, 2), np.float32) if tm is None else tm
    r = extractor(orb).extract(cur, boxes if nbox else None, tm_used, blur if nbox else None)
    kps = r["kps"].astype(KEYPOINT_DTYPE)
    fx, fy, cx, cy = camera_params(w, h)
    kun = O.undistort_keypoints(kps, fx, fy, cx, cy, dist) if dist is not None and dist[0] != 0 else kps.copy()
    # ComputeStereoFromRGBD: the depth under the raw keypoint, uRight from the undistorted x
    _, dep = O.stereo_from_rgbd(kps, depth_float(depth), BF)
    with np.errstate(all="ignore"):
        ur = np.where(dep > 0, kun["x"] - np.float32(BF) / dep, np.float32(-1)).astype(np.float32)
    return dict(tm=tm_used, n_tm=n_tm, blur=blur, kps=kps, kps_un=kun, desc=r["desc"], u_right=ur, depth=dep,
                first=prev is None)


@functools.lru_cache(maxsize=None)
def sequence_ref(name, kind="f32"):
    """frame_ref of every frame of a sequence, frame 0 being a first frame"""
    frames, boxes = sequence(name)
    s = SEQUENCES[name]
    depth = depth_map(s["w"], s["h"], kind)
    return [frame_ref(frames[f - 1] if f else None, frames[f], boxes[f], depth, orb=s["orb"]) for f in range(s["n"])]


@functools.lru_cache(maxsize=None)
def flat_pair(w=160, h=120):
    """Two frames without a corner: goodFeaturesToTrack finds nothing, findFundamentalMat gets no
    point pairs and returns an empty matrix (process_moving_object: None)."""
    a = np.full((h, w), 90, np.uint8)
    b = np.full((h, w), 91, np.uint8)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b
