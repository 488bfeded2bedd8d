"""Python mirror of the reference's front-end interface over the C-ABI (include/coeb_front.h).

  ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
      include/ORBextractor.h:50-51; __call__ mirrors operator() (ORBextractor.h:73-75,
      src/ORBextractor.cc:1088-1342) and returns (keypoints, descriptors) instead of filling
      output arguments.  Accessors GetLevels/GetScaleFactor/... as ORBextractor.h:77-99.
  ORBmatcher(nnratio=0.6, checkOri=True).SearchByProjection(CurrentFrame, LastFrame, th, bMono)
      include/ORBmatcher.h:41,52, src/ORBmatcher.cc:1329-1471; mutates
      CurrentFrame.mvpMapPoints (slot index of the LastFrame MapPoint, -1 = NULL) and returns
      nmatches.
  ORBmatcher(nnratio).SearchByProjection(F, LocalMap, th=3)
      include/ORBmatcher.h:46, src/ORBmatcher.cc:44-129 (the Tracking::SearchLocalPoints call,
      src/Tracking.cc:1222-1271); assigns F.mvpMapPoints[i] = local-map index and returns nmatches.
  ORBmatcher(nnratio, checkOri).SearchByProjection(F, KeyFramePoints, sAlreadyFound, th, ORBdist)
      include/ORBmatcher.h:55, src/ORBmatcher.cc:1473-1600 (Tracking::Relocalization,
      src/Tracking.cc:1531,1545); assigns F.mvpMapPoints[i] = KeyFrame point index.
  ORBmatcher(0.7, True).SearchByBoW(pKF: BowKeyFrame, F)
      include/ORBmatcher.h:65, src/ORBmatcher.cc:159-288 (Tracking::TrackReferenceKeyFrame,
      src/Tracking.cc:833, and Relocalization, :1456); F.ComputeBoW(ctx) first (src/Frame.cc:570-577);
      assigns F.mvpMapPoints[i] = KeyFrame feature index and returns nmatches.
  KeyFrameDatabase(ctx).add / erase / clear / DetectRelocalizationCandidates(F, neighbours) / SearchByBoW(slots, valids, F)
      include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:40-73, 199-309 and the SearchByBoW loop
      of Tracking::Relocalization (src/Tracking.cc:1449-1470); keyframes are named by slot.
      bow_vector(word, weight, node): BowVector::addWeight + normalize(L1).
  Vocabulary.from_text(text) / from_arrays(...)  ORBVocabulary::loadFromTextFile (src/System.cc:72)
  ORBmatcher.DescriptorDistance(a, b)  src/ORBmatcher.cc:1648-1664
  search_local_points(ctx, camera, F, cur_observations, LocalPoints, ...) / track_local_map(...)
      Tracking::SearchLocalPoints from :1246 and Tracking::TrackLocalMap after UpdateLocalMap
      (src/Tracking.cc:996-1047, 1222-1272) on one host frame, one call each; return dicts.
  Context.track_reference_keyframe(camera, F, kf, kf_world_pos, kf_observations, ...)
      Tracking::TrackReferenceKeyFrame (src/Tracking.cc:823-865) on one host frame in one call:
      ComputeBoW, SearchByBoW, the nmatches gate, PoseOptimization and the outlier discard; a dict.
  Optimizer.PoseOptimization(F, camera)  include/Optimizer.h:47, src/Optimizer.cc:239-451; reads
      F.mvpMapPoints (>= 0: has a MapPoint) and F.mvMapPointPos, sets F.mTcw and F.mvbOutlier.

All compute runs in libcoeb_front.so (hand-written gfx950 HIP kernels).  There is no CPU
fallback: importing works anywhere, but constructing an extractor without the built library
or without a gfx950 device raises.
"""
import ctypes as C
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# COEB_LIB_PATH: an alternative build of the same library (kernel experiments); never a fallback
LIB_PATH = os.environ.get("COEB_LIB_PATH") or os.path.join(os.path.dirname(HERE), "lib", "libcoeb_front.so")

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KEYPOINT_DTYPE.itemsize == 28
# one pair of a moving-object batch as coeb_debug_read("flow_pair") returns it (FlowPairRecord, coeb_ctx.hpp)
FLOW_PAIR_PTS = 1024
FLOW_PAIR_DTYPE = np.dtype([("npts", "<i4"), ("nf", "<i4"), ("F", "<f8", (9,)), ("pts", "<f4", (FLOW_PAIR_PTS, 2)),
                            ("nxt", "<f4", (FLOW_PAIR_PTS, 2)), ("status", "u1", (FLOW_PAIR_PTS,)),
                            ("state", "u1", (FLOW_PAIR_PTS,))])
assert FLOW_PAIR_DTYPE.itemsize == 18512
MAX_LEVELS = 16
DEPTH_U16, DEPTH_F32 = 0, 1          # COEB_DEPTH_U16 / COEB_DEPTH_F32

# exported symbols of include/coeb_front.h (checked by tests/test_capi_symbols.py)
ABI_SYMBOLS = [
    "coeb_abi_version", "coeb_create", "coeb_destroy", "coeb_last_error", "coeb_orb_tables_get", "coeb_max_keypoints",
    "coeb_extract", "coeb_extract_batch_device", "coeb_batch_results", "coeb_match_batch_device",
    "coeb_match_batch_device_tcw",
    "coeb_batch_match_results", "coeb_match_lastframe", "coeb_blur_flags", "coeb_stereo_from_rgbd",
    "coeb_rgbd_preprocess", "coeb_descriptor_distance", "coeb_profile_enable", "coeb_profile_read",
    "coeb_profile_reset", "coeb_synchronize", "coeb_device_count", "coeb_debug_read",
    "coeb_device_alloc", "coeb_device_free", "coeb_memcpy_h2d", "coeb_memcpy_d2h", "coeb_set_batch_streams",
    "coeb_match_localmap", "coeb_match_keyframe", "coeb_pose_optimization", "coeb_undistort_keypoints",
    "coeb_boxes_from_int64", "coeb_good_features", "coeb_corner_subpix", "coeb_optical_flow_pyr_lk",
    "coeb_moving_tail", "coeb_moving_object_points", "coeb_moving_object_points_device",
    "coeb_pose_batch_device", "coeb_batch_pose_results",
    "coeb_host_alloc", "coeb_host_free", "coeb_memcpy_h2d_async", "coeb_memcpy_d2h_async",
    "coeb_copyq_create", "coeb_copyq_destroy", "coeb_copyq_h2d", "coeb_copyq_d2h", "coeb_copyq_after_ctx",
    "coeb_ctx_after_copyq", "coeb_copyq_synchronize", "coeb_frame_batch_device", "coeb_batch_frame_results",
    "coeb_track_local_map_batch_device", "coeb_batch_track_results", "coeb_rgbd_preprocess_batch_device",
    "coeb_marker_create", "coeb_marker_destroy", "coeb_marker_record_ctx", "coeb_marker_record_copyq",
    "coeb_ctx_wait_marker", "coeb_copyq_wait_marker", "coeb_marker_synchronize",
    "coeb_tum_read_list", "coeb_tum_associate", "coeb_frame_rgbd",
    "coeb_voc_from_text", "coeb_voc_from_arrays", "coeb_voc_info", "coeb_voc_tables", "coeb_voc_destroy",
    "coeb_bow_set_vocabulary", "coeb_bow_transform", "coeb_bow_batch_device", "coeb_batch_bow_results",
    "coeb_match_bow",
    "coeb_bow_vector", "coeb_kfdb_create", "coeb_kfdb_destroy", "coeb_kfdb_add", "coeb_kfdb_erase", "coeb_kfdb_clear",
    "coeb_kfdb_size", "coeb_kfdb_query", "coeb_match_bow_kfdb", "coeb_kfdb_set_geometry",
    "coeb_kfdb_search_triangulation", "coeb_kfdb_fuse_search", "coeb_kfdb_set_stereo",
    "coeb_kfdb_create_new_map_points",
    "coeb_search_local_points", "coeb_track_local_map", "coeb_track_reference_keyframe",
    "coeb_track_motion_model", "coeb_reloc_refine",
    "coeb_rgbd_stream_create", "coeb_rgbd_stream_destroy", "coeb_rgbd_stream_reset", "coeb_rgbd_stream_frame",
]
# COEB_ABI_VERSION of the include/coeb_front.h these argtypes are written against; lib() refuses
# a library that reports another (tests/test_capi_symbols.py keeps the two equal)
ABI_VERSION = 3


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32)]


class OrbTables(C.Structure):
    _fields_ = [("nlevels", C.c_int32), ("scale_factor", C.c_float),
                ("scale", C.c_float * MAX_LEVELS), ("inv_scale", C.c_float * MAX_LEVELS),
                ("sigma2", C.c_float * MAX_LEVELS), ("inv_sigma2", C.c_float * MAX_LEVELS),
                ("features_per_level", C.c_int32 * MAX_LEVELS), ("umax", C.c_int32 * 16)]


class Camera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]


class LastFrameC(C.Structure):
    _fields_ = [("n", C.c_int32), ("has_mappoint", C.c_void_p), ("outlier", C.c_void_p), ("world_pos", C.c_void_p),
                ("mp_descriptor", C.c_void_p), ("mp_observations", C.c_void_p), ("keys_un", C.c_void_p)]


class CurFrameC(C.Structure):
    _fields_ = [("n", C.c_int32), ("keys_un", C.c_void_p), ("descriptors", C.c_void_p), ("u_right", C.c_void_p)]


class LocalMapC(C.Structure):
    _fields_ = [("n", C.c_int32), ("in_view", C.c_void_p), ("proj_x", C.c_void_p), ("proj_y", C.c_void_p),
                ("proj_xr", C.c_void_p), ("level", C.c_void_p), ("view_cos", C.c_void_p), ("descriptor", C.c_void_p),
                ("observations", C.c_void_p)]


class LocalPointsC(C.Structure):
    _fields_ = [("n", C.c_int32), ("valid", C.c_void_p), ("world_pos", C.c_void_p), ("normal", C.c_void_p),
                ("max_distance", C.c_void_p), ("min_distance", C.c_void_p), ("descriptor", C.c_void_p),
                ("observations", C.c_void_p)]


class TrackFieldsC(C.Structure):
    _fields_ = [("in_view", C.c_void_p), ("proj_x", C.c_void_p), ("proj_y", C.c_void_p), ("proj_xr", C.c_void_p),
                ("level", C.c_void_p), ("view_cos", C.c_void_p)]


class KeyFramePointsC(C.Structure):
    _fields_ = [("n", C.c_int32), ("valid", C.c_void_p), ("world_pos", C.c_void_p), ("descriptor", C.c_void_p),
                ("max_distance", C.c_void_p), ("min_distance", C.c_void_p), ("angle", C.c_void_p)]


class PoseFrameC(C.Structure):
    _fields_ = [("n", C.c_int32), ("has_mappoint", C.c_void_p), ("world_pos", C.c_void_p), ("keys_un", C.c_void_p),
                ("u_right", C.c_void_p)]


class BowKeyFrameC(C.Structure):
    _fields_ = [("n", C.c_int32), ("valid", C.c_void_p), ("descriptor", C.c_void_p), ("node_id", C.c_void_p),
                ("angle", C.c_void_p)]


class RefKeyFrameC(C.Structure):
    _fields_ = [("bow", BowKeyFrameC), ("world_pos", C.c_void_p), ("observations", C.c_void_p)]


class RelocHypothesisC(C.Structure):
    _fields_ = [("kf", KeyFramePointsC), ("match", C.c_void_p), ("inlier", C.c_void_p), ("Tcw", C.c_float * 16)]


RELOC_MAX_HYP = 16      # COEB_RELOC_MAX_HYP


class VoPointsC(C.Structure):
    _fields_ = [("depth", C.c_void_p), ("descriptors", C.c_void_p), ("th_depth", C.c_float),
                ("created_out", C.c_void_p), ("created_pos", C.c_void_p)]


VO_MAX_LAST = 16384     # COEB_VO_MAX_LAST


class BowFrameC(C.Structure):
    _fields_ = [("n", C.c_int32), ("descriptor", C.c_void_p), ("node_id", C.c_void_p), ("angle", C.c_void_p)]


class KfdbKeyFrameC(C.Structure):
    _fields_ = [("n", C.c_int32), ("descriptor", C.c_void_p), ("node_id", C.c_void_p), ("angle", C.c_void_p),
                ("bow_word", C.c_void_p), ("bow_value", C.c_void_p), ("nw", C.c_int32)]


class FusePointsC(C.Structure):
    _fields_ = [("n", C.c_int32), ("valid", C.c_void_p), ("world_pos", C.c_void_p), ("normal", C.c_void_p),
                ("max_distance", C.c_void_p), ("min_distance", C.c_void_p), ("descriptor", C.c_void_p)]


class FuseJobC(C.Structure):
    _fields_ = [("slot", C.c_int32), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3),
                ("first", C.c_int32), ("count", C.c_int32), ("skip", C.c_void_p)]


FUSE_MAX_JOBS = 128     # COEB_FUSE_MAX_JOBS


class RgbdStreamOutC(C.Structure):
    _fields_ = [("tm_xy", C.c_void_p), ("tm_cap", C.c_int), ("n_tm", C.c_int), ("blur_flag", C.c_void_p),
                ("gray", C.c_void_p), ("gray_stride", C.c_size_t), ("kp", C.c_void_p), ("kp_un", C.c_void_p),
                ("desc", C.c_void_p), ("u_right", C.c_void_p), ("depth", C.c_void_p), ("cap", C.c_int), ("n", C.c_int),
                ("first", C.c_int)]


STREAM_NO_SHADOW = 1    # COEB_STREAM_NO_SHADOW
STREAM_TM_CAP = 1024    # T_M points a stream frame can return


class CoebError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libcoeb_front.so (in-tree build); raise if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CoebError("libcoeb_front.so not built (run __graft_entry__.build() or make -C coeb-slam_amd/csrc)")
        L = C.CDLL(LIB_PATH)
        got = L.coeb_abi_version()
        if got != ABI_VERSION:
            raise CoebError("%s reports ABI %d, this binding is written for ABI %d (rebuild the library)"
                            % (LIB_PATH, got, ABI_VERSION))
        L.coeb_create.restype = C.c_void_p
        L.coeb_create.argtypes = [C.POINTER(OrbParams), C.c_int, C.c_int, C.c_int, C.c_int]
        L.coeb_destroy.argtypes = [C.c_void_p]
        L.coeb_last_error.restype = C.c_char_p
        L.coeb_last_error.argtypes = [C.c_void_p]
        L.coeb_orb_tables_get.argtypes = [C.c_void_p, C.POINTER(OrbTables)]
        L.coeb_max_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.coeb_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                   C.POINTER(C.c_int)]
        L.coeb_frame_rgbd.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t,
                                      C.c_int, C.c_float, C.POINTER(Camera), C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.coeb_extract_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.coeb_frame_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p]
        L.coeb_batch_frame_results.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                               C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
        L.coeb_batch_results.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
        L.coeb_match_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Camera),
                                              C.c_void_p, C.c_float, C.c_int32]
        L.coeb_match_batch_device_tcw.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                  C.POINTER(Camera), C.c_void_p, C.c_float, C.c_int32]
        L.coeb_batch_match_results.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.coeb_pose_batch_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int, C.c_void_p, C.c_int32]
        L.coeb_batch_pose_results.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_void_p)]
        L.coeb_track_local_map_batch_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int, C.c_int32, C.c_float,
                                                        C.c_float]
        L.coeb_batch_track_results.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 6
        L.coeb_rgbd_preprocess_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                        C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.coeb_match_lastframe.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(CurFrameC),
                                           C.POINTER(LastFrameC), C.c_void_p, C.c_void_p, C.c_float, C.c_int,
                                           C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.coeb_match_localmap.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(CurFrameC), C.c_void_p,
                                          C.POINTER(LocalMapC), C.c_float, C.c_float, C.c_void_p, C.POINTER(C.c_int)]
        L.coeb_search_local_points.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(CurFrameC), C.c_void_p,
                                               C.c_void_p, C.POINTER(LocalPointsC), C.c_float, C.c_float, C.c_float,
                                               C.POINTER(TrackFieldsC), C.c_void_p, C.POINTER(C.c_int),
                                               C.POINTER(C.c_int)]
        L.coeb_track_local_map.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(CurFrameC), C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.POINTER(LocalPointsC), C.c_float, C.c_float, C.c_float,
                                           C.c_int, C.POINTER(TrackFieldsC), C.c_void_p, C.c_void_p] + \
            [C.POINTER(C.c_int)] * 4
        L.coeb_track_reference_keyframe.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(CurFrameC), C.c_void_p,
                                                    C.c_int, C.POINTER(RefKeyFrameC), C.c_void_p, C.c_float, C.c_int,
                                                    C.c_int] + [C.c_void_p] * 5 + [C.POINTER(C.c_int)] * 4
        L.coeb_track_motion_model.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(CurFrameC),
                                              C.POINTER(LastFrameC), C.POINTER(VoPointsC), C.c_void_p, C.c_void_p,
                                              C.c_float, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3 + \
            [C.POINTER(C.c_int)] * 4
        L.coeb_reloc_refine.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(CurFrameC),
                                        C.POINTER(RelocHypothesisC), C.c_int, C.c_float, C.c_int, C.c_float, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.POINTER(C.c_int)]
        L.coeb_match_keyframe.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(CurFrameC), C.c_void_p,
                                          C.POINTER(KeyFramePointsC), C.c_void_p, C.c_float, C.c_int, C.c_int,
                                          C.c_void_p, C.POINTER(C.c_int)]
        L.coeb_pose_optimization.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(PoseFrameC), C.c_void_p,
                                             C.c_void_p, C.POINTER(C.c_int)]
        L.coeb_undistort_keypoints.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_void_p]
        L.coeb_boxes_from_int64.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.coeb_good_features.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_double,
                                         C.c_double, C.c_double, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.coeb_corner_subpix.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int,
                                         C.c_int, C.c_int, C.c_double]
        L.coeb_optical_flow_pyr_lk.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t,
                                               C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                               C.c_void_p, C.c_void_p]
        L.coeb_moving_tail.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                       C.c_void_p, C.POINTER(C.c_int)]
        L.coeb_moving_object_points.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t,
                                                C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p]
        L.coeb_moving_object_points_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                       C.c_size_t, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                                       C.c_void_p]
        L.coeb_blur_flags.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int,
                                      C.c_void_p]
        L.coeb_stereo_from_rgbd.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                            C.c_size_t, C.c_float, C.c_void_p, C.c_void_p]
        L.coeb_rgbd_preprocess.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                           C.c_size_t, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.coeb_descriptor_distance.argtypes = [C.c_void_p, C.c_void_p]
        L.coeb_tum_read_list.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.POINTER(C.c_int)]
        L.coeb_tum_associate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double,
                                         C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.coeb_voc_from_text.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.coeb_voc_from_arrays.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_void_p)]
        L.coeb_voc_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 4
        L.coeb_voc_tables.argtypes = [C.c_void_p] * 9
        L.coeb_voc_destroy.restype = None
        L.coeb_voc_destroy.argtypes = [C.c_void_p]
        L.coeb_bow_set_vocabulary.argtypes = [C.c_void_p, C.c_void_p]
        L.coeb_bow_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.coeb_bow_batch_device.argtypes = [C.c_void_p, C.c_int]
        L.coeb_batch_bow_results.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.coeb_match_bow.argtypes = [C.c_void_p, C.POINTER(BowKeyFrameC), C.POINTER(BowFrameC), C.c_float, C.c_int,
                                     C.c_void_p, C.POINTER(C.c_int)]
        L.coeb_bow_vector.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_int, C.POINTER(C.c_int)]
        L.coeb_kfdb_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.coeb_kfdb_destroy.restype = None
        L.coeb_kfdb_destroy.argtypes = [C.c_void_p]
        L.coeb_kfdb_add.argtypes = [C.c_void_p, C.POINTER(KfdbKeyFrameC), C.POINTER(C.c_int)]
        L.coeb_kfdb_erase.argtypes = [C.c_void_p, C.c_int]
        L.coeb_kfdb_clear.argtypes = [C.c_void_p]
        L.coeb_kfdb_size.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.coeb_kfdb_query.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.coeb_match_bow_kfdb.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(BowFrameC),
                                          C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        L.coeb_kfdb_set_geometry.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.coeb_kfdb_search_triangulation.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                     C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                     C.c_void_p, C.c_void_p]
        L.coeb_kfdb_set_stereo.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.coeb_kfdb_create_new_map_points.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                      C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.coeb_kfdb_fuse_search.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(FusePointsC), C.POINTER(FuseJobC),
                                            C.c_int, C.c_float, C.c_void_p, C.c_void_p]
        L.coeb_profile_enable.argtypes = [C.c_void_p, C.c_int]
        L.coeb_profile_reset.argtypes = [C.c_void_p]
        L.coeb_profile_read.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                        C.POINTER(C.c_int)]
        L.coeb_synchronize.argtypes = [C.c_void_p]
        L.coeb_set_batch_streams.argtypes = [C.c_void_p, C.c_int]
        L.coeb_device_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.coeb_device_free.argtypes = [C.c_void_p, C.c_void_p]
        L.coeb_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.coeb_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.coeb_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
        L.coeb_host_free.argtypes = [C.c_void_p]
        L.coeb_memcpy_h2d_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.coeb_memcpy_d2h_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.coeb_copyq_create.restype = C.c_void_p
        L.coeb_copyq_create.argtypes = [C.c_void_p]
        L.coeb_copyq_destroy.argtypes = [C.c_void_p]
        L.coeb_copyq_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.coeb_copyq_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.coeb_copyq_after_ctx.argtypes = [C.c_void_p, C.c_void_p]
        L.coeb_ctx_after_copyq.argtypes = [C.c_void_p, C.c_void_p]
        L.coeb_copyq_synchronize.argtypes = [C.c_void_p]
        L.coeb_marker_create.restype = C.c_void_p
        L.coeb_marker_create.argtypes = [C.c_void_p]
        for nm in ("coeb_marker_destroy", "coeb_marker_synchronize"):
            getattr(L, nm).argtypes = [C.c_void_p]
        for nm in ("coeb_marker_record_ctx", "coeb_marker_record_copyq", "coeb_ctx_wait_marker",
                   "coeb_copyq_wait_marker"):
            getattr(L, nm).argtypes = [C.c_void_p, C.c_void_p]
        L.coeb_debug_read.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_size_t)]
        L.coeb_rgbd_stream_create.argtypes = [C.c_void_p, C.c_uint, C.POINTER(C.c_void_p)]
        L.coeb_rgbd_stream_destroy.restype = None
        L.coeb_rgbd_stream_destroy.argtypes = [C.c_void_p]
        L.coeb_rgbd_stream_reset.argtypes = [C.c_void_p]
        L.coeb_rgbd_stream_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.POINTER(Camera), C.c_void_p,
                                             C.c_void_p, C.c_int, C.POINTER(RgbdStreamOutC)]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class Vocabulary:
    """ORBVocabulary as plain data (host only, no device needed): a k-ary tree of 32-byte
    descriptors with a weight per word.  Parity against DBoW2 itself is unpinned."""

    def __init__(self, handle):
        self.h = C.c_void_p(handle)

    @classmethod
    def from_text(cls, text):
        """ORBvoc.txt's text (bytes or str); raises CoebError (COEB_EINVAL) on a malformed file."""
        if isinstance(text, str):
            text = text.encode()
        h = C.c_void_p()
        rc = lib().coeb_voc_from_text(text, len(text), C.byref(h))
        if rc:
            raise CoebError("coeb_voc_from_text rc=%d" % rc)
        return cls(h.value)

    @classmethod
    def from_arrays(cls, k, L, parent, is_leaf, desc, weight):
        """Node i + 1 = (parent[i], is_leaf[i], desc[i], weight[i]); node 0 is the root."""
        parent = np.ascontiguousarray(parent, np.int32)
        n = len(parent)
        is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(n, 32)
        weight = np.ascontiguousarray(weight, np.float64)
        if len(is_leaf) != n or len(weight) != n:
            raise ValueError("Vocabulary arrays differ in length")
        h = C.c_void_p()
        rc = lib().coeb_voc_from_arrays(k, L, n, _p(parent), _p(is_leaf), _p(desc), _p(weight), C.byref(h))
        if rc:
            raise CoebError("coeb_voc_from_arrays rc=%d" % rc)
        return cls(h.value)

    def info(self):
        """(k, L, nodes with the root, words)"""
        v = [C.c_int() for _ in range(4)]
        lib().coeb_voc_info(self.h, *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    def tables(self):
        """The tables the device walks, by slot (include/coeb_front.h, coeb_voc_tables)."""
        _, _, nn, nw = self.info()
        t = dict(child_first=np.empty(nn, np.int32), child_count=np.empty(nn, np.int32), word=np.empty(nn, np.int32),
                 node_id=np.empty(nn, np.int32), positive=np.empty(nn, np.uint8), desc=np.empty((nn, 32), np.uint8),
                 word_weight=np.empty(nw, np.float64), word_node=np.empty(nw, np.int32))
        lib().coeb_voc_tables(self.h, *[_p(t[k]) for k in ("child_first", "child_count", "word", "node_id", "positive",
                                                            "desc", "word_weight", "word_node")])
        return t

    def close(self):
        if getattr(self, "h", None):
            lib().coeb_voc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One coeb_ctx: device buffers + HIP stream of one host thread (not reentrant)."""

    def __init__(self, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, device=0,
                 max_width=1280, max_height=960, max_batch=1):
        L = lib()
        self.params = OrbParams(nfeatures, scale_factor, nlevels, ini_th, min_th)
        h = L.coeb_create(C.byref(self.params), device, max_width, max_height, max_batch)
        if not h:
            raise CoebError(L.coeb_last_error(None).decode())
        self.h = C.c_void_p(h)
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            lib().coeb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != 0:
            raise CoebError("coeb rc=%d: %s" % (rc, lib().coeb_last_error(self.h).decode()))
        return rc

    def tables(self):
        t = OrbTables()
        self.check(lib().coeb_orb_tables_get(self.h, C.byref(t)))
        return t

    def max_keypoints(self, w, h):
        cache = self.__dict__.setdefault("_kcap", {})
        r = cache.get((w, h))
        if r is None:
            r = lib().coeb_max_keypoints(self.h, w, h)
            if r < 0:
                self.check(r)
            cache[(w, h)] = r
        return r

    # ---- single frame (host buffers) ----
    def extract(self, gray, boxes=None, tm=None, blur=None):
        gray = np.ascontiguousarray(gray, np.uint8)
        if gray.size == 0:
            return np.zeros(0, KEYPOINT_DTYPE), None
        h, w = gray.shape
        boxes = None if boxes is None else np.ascontiguousarray(boxes, np.float32)
        tm = None if tm is None else np.ascontiguousarray(tm, np.float32)
        blur = None if blur is None else np.ascontiguousarray(blur, np.int32)
        nb = 0 if boxes is None else len(boxes)
        nt = 0 if tm is None else len(tm)
        nf = 0 if blur is None else len(blur)
        cap = self.max_keypoints(w, h)
        # outputs written by the call (no zero fill) and returned as their first n rows (no copy):
        # the per-call cost of the binding is part of the drop-in latency bench.py measures
        kps = np.empty(cap, KEYPOINT_DTYPE)
        desc = np.empty((cap, 32), np.uint8)
        n = C.c_int()
        self.check(lib().coeb_extract(self.h, _p(gray), w, h, w, _p(boxes) if nb else None, nb,
                                      _p(tm) if nt else None, nt, _p(blur) if nf else None,
                                      nf, _p(kps), _p(desc), cap, C.byref(n)))
        n = n.value
        return kps[:n], (desc[:n] if n else None)

    def frame_rgbd(self, gray, depth, cam, dist=None, boxes=None, tm=None, blur=None, depth_scale=1.0):
        """The RGB-D Frame constructor's tail (Frame.cc:214-223) in one call: extraction,
        UndistortKeyPoints with dist = mDistCoef (k1, k2, p1, p2[, k3]; None copies the keys) and
        ComputeStereoFromRGBD on depth ((H, W) float32, or uint16 with depth_scale =
        mDepthMapFactor).  Returns dict(kps, kps_un, desc, u_right, depth)."""
        gray = np.ascontiguousarray(gray, np.uint8)
        if gray.size == 0:
            return dict(kps=np.zeros(0, KEYPOINT_DTYPE), kps_un=np.zeros(0, KEYPOINT_DTYPE), desc=None,
                        u_right=np.zeros(0, np.float32), depth=np.zeros(0, np.float32))
        h, w = gray.shape
        depth = np.ascontiguousarray(depth)
        if depth.shape != (h, w) or depth.dtype not in (np.uint16, np.float32):
            raise ValueError("depth must be (H, W) uint16 or float32")
        dtype = DEPTH_F32 if depth.dtype == np.float32 else DEPTH_U16
        d = None
        if dist is not None:
            d = np.zeros(5, np.float32)
            d[:len(dist)] = np.asarray(dist, np.float32)
        boxes = None if boxes is None else np.ascontiguousarray(boxes, np.float32)
        tm = None if tm is None else np.ascontiguousarray(tm, np.float32)
        blur = None if blur is None else np.ascontiguousarray(blur, np.int32)
        nb = 0 if boxes is None else len(boxes)
        nt = 0 if tm is None else len(tm)
        nf = 0 if blur is None else len(blur)
        cap = self.max_keypoints(w, h)
        kps, kun = np.empty(cap, KEYPOINT_DTYPE), np.empty(cap, KEYPOINT_DTYPE)
        desc = np.empty((cap, 32), np.uint8)
        ur, dep = np.empty(cap, np.float32), np.empty(cap, np.float32)
        n = C.c_int()
        self.check(lib().coeb_frame_rgbd(self.h, _p(gray), w, h, w, _p(depth), depth.strides[0], dtype,
                                         C.c_float(depth_scale), C.byref(cam), _p(d), _p(boxes) if nb else None, nb,
                                         _p(tm) if nt else None, nt, _p(blur) if nf else None, nf, _p(kps), _p(kun),
                                         _p(desc), _p(ur), _p(dep), cap, C.byref(n)))
        n = n.value
        return dict(kps=kps[:n], kps_un=kun[:n], desc=(desc[:n] if n else None), u_right=ur[:n], depth=dep[:n])

    # ---- bag of words ----
    def set_vocabulary(self, voc):
        self.check(lib().coeb_bow_set_vocabulary(self.h, voc.h))

    def bow_transform(self, desc, levelsup=4):
        """Frame::ComputeBoW (Frame.cc:570-577) for n x 32 descriptors: dict(word, node, weight,
        fv_node, fv_off, fv_idx) -- word ids, FeatureVector node ids (-1: word weight not > 0),
        word weights, and the FeatureVector as a CSR (node ids ascending, indices ascending)."""
        desc = np.zeros((0, 32), np.uint8) if desc is None else np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        m = max(n, 1)
        word, node, weight = np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m, np.float64)
        fv_node, fv_off, fv_idx = np.empty(m, np.int32), np.empty(m + 1, np.int32), np.empty(m, np.int32)
        nfv = C.c_int()
        self.check(lib().coeb_bow_transform(self.h, _p(desc) if n else None, n, levelsup, _p(word), _p(node),
                                            _p(weight), _p(fv_node), _p(fv_off), _p(fv_idx), m, C.byref(nfv)))
        nd = nfv.value
        return dict(word=word[:n], node=node[:n], weight=weight[:n], fv_node=fv_node[:nd], fv_off=fv_off[:nd + 1],
                    fv_idx=fv_idx[:int(fv_off[nd])])

    def track_reference_keyframe(self, camera, F, kf, kf_world_pos, kf_observations, cur_node_id=None, levelsup=4,
                                 nnratio=0.7, check_orientation=True, min_matches=15):
        """Tracking::TrackReferenceKeyFrame (src/Tracking.cc:823-865) in one call
        (coeb_track_reference_keyframe): ComputeBoW of F.mDescriptors (skipped when cur_node_id, the
        F.mFeatVec node per feature, is given), SearchByBoW against kf (a BowKeyFrame whose matched
        MapPoints sit at kf_world_pos with kf_observations), the nmatches < min_matches gate,
        PoseOptimization from F.mTcw (mLastFrame.mTcw) and the outlier discard.  F is not modified.
        Returns a dict: word, node, weight (None when cur_node_id was given), match (i32[F.N],
        KeyFrame index or -1, after the discard), discarded (i32[F.N], the KeyFrame index a discarded
        keypoint had, else -1), Tcw (4x4 f32), nmatches_bow, ninliers_pose, nmatches, nmatches_map."""
        n, m = F.N, max(F.N, 1)
        cf = CurFrameC(n, C.c_void_p(F.mvKeysUn.ctypes.data), C.c_void_p(F.mDescriptors.ctypes.data),
                       C.c_void_p(F.mvuRight.ctypes.data))
        xw = np.ascontiguousarray(kf_world_pos, np.float32).reshape(kf.N, 3)
        nobs = np.ascontiguousarray(kf_observations, np.int32)
        if len(nobs) != kf.N:
            raise ValueError("track_reference_keyframe: keyframe arrays differ in length")
        kc = RefKeyFrameC(BowKeyFrameC(kf.N, *[C.c_void_p(a.ctypes.data) for a in (kf.valid, kf.descriptor, kf.node_id,
                                                                                 kf.angle)]),
                          C.c_void_p(xw.ctypes.data), C.c_void_p(nobs.ctypes.data))
        cnode = None if cur_node_id is None else np.ascontiguousarray(cur_node_id, np.int32)
        if cnode is not None and len(cnode) != n:
            raise ValueError("track_reference_keyframe: cur_node_id must have F.N entries")
        if cnode is not None and n == 0:
            cnode = np.zeros(1, np.int32)               # an empty frame still says "mBowVec is filled": not NULL
        word, node, weight = ((np.empty(m, np.int32), np.empty(m, np.int32), np.empty(m, np.float64))
                              if cnode is None else (None, None, None))
        T = np.ascontiguousarray(F.mTcw, np.float32).copy()
        match, disc = np.full(m, -1, np.int32), np.full(m, -1, np.int32)
        nb, nin, nm, nmap = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self.check(lib().coeb_track_reference_keyframe(
            self.h, C.byref(camera), C.byref(cf), _p(cnode), levelsup, C.byref(kc), _p(T), nnratio, int(bool(check_orientation)), int(min_matches), _p(word), _p(node),
            _p(weight), _p(match), _p(disc), C.byref(nb), C.byref(nin), C.byref(nm), C.byref(nmap)))
        cut = lambda a: None if a is None else a[:n]
        return dict(word=cut(word), node=cut(node), weight=cut(weight), match=match[:n], discarded=disc[:n],
                    Tcw=T.reshape(4, 4), nmatches_bow=nb.value, ninliers_pose=nin.value, nmatches=nm.value,
                    nmatches_map=nmap.value)

    def track_with_motion_model(self, camera, F, LastFrame, th=15.0, bMono=False, check_orientation=True,
                                min_matches=20, depth=None, th_depth=None):
        """Tracking::TrackWithMotionModel (src/Tracking.cc:933-994) in one call
        (coeb_track_motion_model): SearchByProjection(F, LastFrame, th, bMono) from F.mTcw (the
        caller's mVelocity * mLastFrame.mTcw), the 2*th retry and the gate at min_matches,
        PoseOptimization and the outlier discard.  LastFrame is a Frame with map_points as
        ORBmatcher.SearchByProjection takes it.  depth (LastFrame.mvDepth) with th_depth (mThDepth)
        selects localisation mode: UpdateLastFrame's visual-odometry points (:878-930) are created
        on the device first, with LastFrame.mDescriptors as their descriptors.  Neither frame is
        modified.  Returns a dict: match (i32[F.N], LastFrame slot or -1, after the discard),
        discarded (i32[F.N], the slot a discarded keypoint had, else -1), outlier (u8[F.N], the
        optimiser's flags), Tcw (4x4 f32), nmatches_search, ninliers_pose, nmatches, nmatches_map,
        and in localisation mode created (u8[LastFrame.N]) and created_pos (f32[LastFrame.N, 3],
        zero where nothing was created), else None for both."""
        n, m = F.N, max(F.N, 1)
        nl = LastFrame.N
        mp = LastFrame.map_points
        has = np.ascontiguousarray(mp["valid"], np.uint8)
        outl = np.ascontiguousarray(LastFrame.mvbOutlier, np.uint8)
        xw = np.ascontiguousarray(mp["world_pos"], np.float32).reshape(nl, 3)
        desc = np.ascontiguousarray(mp["descriptor"], np.uint8).reshape(nl, 32)
        nobs = np.ascontiguousarray(mp["observations"], np.int32)
        keys = np.ascontiguousarray(LastFrame.mvKeysUn)
        if not (len(has) == len(outl) == len(nobs) == nl):
            raise ValueError("track_with_motion_model: LastFrame arrays differ in length")
        lf = LastFrameC(nl, has.ctypes.data, outl.ctypes.data, xw.ctypes.data, desc.ctypes.data, nobs.ctypes.data,
                        keys.ctypes.data)
        cf = CurFrameC(n, C.c_void_p(F.mvKeysUn.ctypes.data), C.c_void_p(F.mDescriptors.ctypes.data),
                       C.c_void_p(F.mvuRight.ctypes.data))
        vo = created = cpos = None
        if depth is not None:
            if th_depth is None:
                raise ValueError("track_with_motion_model: depth without th_depth")
            z = np.ascontiguousarray(depth, np.float32)
            if len(z) != nl:
                raise ValueError("track_with_motion_model: depth must have LastFrame.N entries")
            created, cpos = np.zeros(max(nl, 1), np.uint8), np.zeros((max(nl, 1), 3), np.float32)
            vo = VoPointsC(z.ctypes.data, LastFrame.mDescriptors.ctypes.data, float(th_depth), created.ctypes.data,
                           cpos.ctypes.data)
        T = np.ascontiguousarray(F.mTcw, np.float32).copy()
        Tl = np.ascontiguousarray(LastFrame.mTcw, np.float32)
        match, disc, out = np.full(m, -1, np.int32), np.full(m, -1, np.int32), np.zeros(m, np.uint8)
        ns, nin, nm, nmap = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self.check(lib().coeb_track_motion_model(
            self.h, C.byref(camera), C.byref(cf), C.byref(lf), None if vo is None else C.byref(vo), _p(Tl), _p(T), th,
            int(bool(bMono)), int(bool(check_orientation)), int(min_matches), _p(match), _p(disc), _p(out),
            C.byref(ns), C.byref(nin), C.byref(nm), C.byref(nmap)))
        return dict(match=match[:n], discarded=disc[:n], outlier=out[:n], Tcw=T.reshape(4, 4),
                    nmatches_search=ns.value, ninliers_pose=nin.value, nmatches=nm.value, nmatches_map=nmap.value,
                    created=None if created is None else created[:nl], created_pos=None if cpos is None else cpos[:nl])

    def reloc_refine(self, camera, F, hypotheses, th1=10.0, orb_dist1=100, th2=3.0, orb_dist2=64,
                     check_orientation=True, min_good=10, low_good=30, enough_good=50):
        """Tracking::Relocalization behind PnPsolver::iterate (src/Tracking.cc:1502-1565) for the
        hypotheses of one round in one call (coeb_reloc_refine).  F: the current Frame (its mTcw and
        mvpMapPoints are not read or modified).  hypotheses: up to RELOC_MAX_HYP tuples (kf, match,
        inlier, Tcw): the candidate's KeyFramePoints (valid = pMP && !isBad() only), the KeyFrame
        index SearchByBoW gave each keypoint (i32[F.N], -1: none), vbInliers (u8[F.N]) and the PnP
        pose.  Returns a dict over the H hypotheses: match (i32[H, F.N], the KeyFrame index
        mvpMapPoints holds or -1), outlier (u8[H, F.N], mvbOutlier where the keypoint held a point
        at the last optimisation that ran, else 0), Tcw (f32[H, 4, 4]), ngood, nadditional1,
        nadditional2, stage (i32[H] each) and first_good (the lowest h with ngood >= enough_good,
        or -1)."""
        n, H = F.N, len(hypotheses)
        keep, hy = [], (RelocHypothesisC * max(H, 1))()
        for h, (kf, match, inlier, Tcw) in enumerate(hypotheses):
            m = np.ascontiguousarray(match, np.int32)
            inl = np.ascontiguousarray(inlier, np.uint8)
            if len(m) != n or len(inl) != n:
                raise ValueError("reloc_refine: match / inlier must have F.N entries")
            keep.append((m, inl))
            hy[h].kf = KeyFramePointsC(kf.N, *[C.c_void_p(a.ctypes.data) for a in (
                kf.valid, kf.world_pos, kf.descriptor, kf.max_distance, kf.min_distance, kf.angle)])
            hy[h].match, hy[h].inlier = m.ctypes.data, inl.ctypes.data
            C.memmove(hy[h].Tcw, np.ascontiguousarray(Tcw, np.float32).ctypes.data, 64)
        cf = CurFrameC(n, C.c_void_p(F.mvKeysUn.ctypes.data), C.c_void_p(F.mDescriptors.ctypes.data),
                       C.c_void_p(F.mvuRight.ctypes.data))
        match = np.full((max(H, 1), n), -1, np.int32)
        out = np.zeros((max(H, 1), n), np.uint8)
        cnt = [np.zeros(max(H, 1), np.int32) for _ in range(4)]
        first = C.c_int(-1)
        pad = lambda a: a if a.size else np.zeros(1, a.dtype)       # a valid address for an empty array
        m_, o_ = pad(match), pad(out)
        self.check(lib().coeb_reloc_refine(
            self.h, C.byref(camera), C.byref(cf), hy, H, th1, int(orb_dist1), th2, int(orb_dist2),
            int(bool(check_orientation)), int(min_good), int(low_good), int(enough_good), _p(m_), _p(o_),
            *[_p(a) for a in cnt], C.byref(first)))
        T = np.zeros((H, 4, 4), np.float32)
        for h in range(H):
            C.memmove(T[h].ctypes.data, hy[h].Tcw, 64)
        return dict(match=match[:H], outlier=out[:H], Tcw=T, ngood=cnt[0][:H], nadditional1=cnt[1][:H],
                    nadditional2=cnt[2][:H], stage=cnt[3][:H], first_good=first.value)

    def bow_batch_device(self, levelsup=4):
        """The transform over the last extracted batch; results: batch_bow_results()."""
        self.check(lib().coeb_bow_batch_device(self.h, levelsup))

    def batch_bow_results(self):
        """Device pointers (word ids, node ids), each [nframes][kcap] int32."""
        w, nd = C.c_void_p(), C.c_void_p()
        self.check(lib().coeb_batch_bow_results(self.h, C.byref(w), C.byref(nd)))
        return w.value, nd.value

    # ---- device-resident batch ----
    def extract_batch_device(self, d_gray_ptr, nframes, w, h, boxes=None, box_off=None, tm=None, tm_off=None,
                             blur=None):
        args = []
        keep = []
        for a, dt in ((boxes, np.float32), (box_off, np.int32), (tm, np.float32), (tm_off, np.int32),
                      (blur, np.int32)):
            if a is None:
                args.append(None)
            else:
                a = np.ascontiguousarray(a, dt)
                keep.append(a)
                args.append(_p(a))
        self.check(lib().coeb_extract_batch_device(self.h, C.c_void_p(d_gray_ptr), nframes, w, h, *args))

    def frame_batch_device(self, d_gray_ptr, nframes, w, h, boxes=None, box_off=None):
        """The RGB-D Frame constructor on the batch (coeb_frame_batch_device): T_M from the previous
        frame, box blur flags and the masked extraction, all on the device."""
        b = None if boxes is None else np.ascontiguousarray(boxes, np.float32)
        o = None if box_off is None else np.ascontiguousarray(box_off, np.int32)
        self.check(lib().coeb_frame_batch_device(self.h, C.c_void_p(d_gray_ptr), nframes, w, h, _p(b), _p(o)))

    def batch_frame_results(self, nframes, nbox=0):
        """Host copies of the last frame batch's T_M (list of (n, 2) arrays, None where F was
        empty) and blur flags (nbox,)."""
        tm, ntm, cap, blur = C.c_void_p(), C.c_void_p(), C.c_int(), C.c_void_p()
        self.check(lib().coeb_batch_frame_results(self.h, C.byref(tm), C.byref(ntm), C.byref(cap), C.byref(blur)))
        n = self.download(ntm.value, 4 * nframes, np.int32)
        pts = self.download(tm.value, 8 * cap.value * nframes, np.float32).reshape(nframes, cap.value, 2)
        tms = [None if n[f] < 0 else pts[f, :n[f]].copy() for f in range(nframes)]
        flags = self.download(blur.value, 4 * nbox, np.int32) if nbox and blur.value else np.zeros(0, np.int32)
        return tms, flags

    def batch_results(self):
        k, d, n = C.c_void_p(), C.c_void_p(), C.c_void_p()
        cap = C.c_int()
        self.check(lib().coeb_batch_results(self.h, C.byref(k), C.byref(d), C.byref(n), C.byref(cap)))
        return k.value, d.value, n.value, cap.value

    def match_batch_device(self, d_depth_ptr, nframes, w, h, cam, Tcw, th=15.0, nobs=2):
        Tcw = np.ascontiguousarray(Tcw, np.float32)
        self.check(lib().coeb_match_batch_device(self.h, C.c_void_p(d_depth_ptr), nframes, w, h, C.byref(cam),
                                                 _p(Tcw), th, nobs))

    def match_batch_device_tcw(self, d_depth_ptr, nframes, w, h, cam, d_tcw_ptr, th=15.0, nobs=2):
        """As match_batch_device, with the (nframes, 4, 4) poses already in device memory."""
        self.check(lib().coeb_match_batch_device_tcw(self.h, C.c_void_p(d_depth_ptr), nframes, w, h, C.byref(cam),
                                                     C.c_void_p(d_tcw_ptr), th, nobs))

    def batch_match_results(self):
        m, n = C.c_void_p(), C.c_void_p()
        self.check(lib().coeb_batch_match_results(self.h, C.byref(m), C.byref(n)))
        return m.value, n.value

    def pose_batch_device(self, cam, nframes, d_tcw_ptr, min_matches=20):
        """TrackWithMotionModel's PoseOptimization over the batch matched last (Tracking.cc:947-964)."""
        self.check(lib().coeb_pose_batch_device(self.h, C.byref(cam), nframes, C.c_void_p(d_tcw_ptr), min_matches))

    def batch_pose_results(self):
        t, n, o = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.check(lib().coeb_batch_pose_results(self.h, C.byref(t), C.byref(n), C.byref(o)))
        return t.value, n.value, o.value

    def track_local_map_batch_device(self, cam, nframes, nkf=2, th=3.0, nnratio=0.8):
        """Tracking::TrackLocalMap over the batch posed last (coeb_track_local_map_batch_device):
        outlier discard, local map of KeyFrames f-1 / f-2 through isInFrustum, the local-map
        SearchByProjection(th = 3 for RGB-D, Tracking.cc:1264-1270), second PoseOptimization."""
        self.check(lib().coeb_track_local_map_batch_device(self.h, C.byref(cam), nframes, int(nkf), float(th),
                                                           float(nnratio)))

    def rgbd_preprocess_batch_device(self, d_img, channels, rgb_order, d_depth, depth_type, depth_scale, nframes, w, h,
                                     d_gray, d_depth_out):
        """GrabImageRGBD's cvtColor + depth convertTo over a packed device batch."""
        self.check(lib().coeb_rgbd_preprocess_batch_device(self.h, C.c_void_p(d_img), channels, rgb_order,
                                                           C.c_void_p(d_depth), depth_type, float(depth_scale), nframes,
                                                           w, h, C.c_void_p(d_gray), C.c_void_p(d_depth_out)))

    def batch_track_results(self):
        """Device pointers (Tcw, ninliers, nmatches_map, nlocal, local_match, outlier)."""
        ps = [C.c_void_p() for _ in range(6)]
        self.check(lib().coeb_batch_track_results(self.h, *[C.byref(p) for p in ps]))
        return tuple(p.value for p in ps)

    def synchronize(self):
        self.check(lib().coeb_synchronize(self.h))

    def set_batch_streams(self, n):
        """HIP streams a batch is chunked over (1 = serial on the context stream)."""
        self.check(lib().coeb_set_batch_streams(self.h, int(n)))

    def debug_read(self, what, f=0):
        size = C.c_size_t()
        self.check(lib().coeb_debug_read(self.h, what.encode(), f, None, 0, C.byref(size)))
        buf = np.zeros(size.value, np.uint8)
        self.check(lib().coeb_debug_read(self.h, what.encode(), f, _p(buf), size.value, C.byref(size)))
        return buf

    def flow_pair(self, z):
        """Pair z (frames z, z + 1) of the last moving-object batch, from the flow scratch
        (coeb_debug_read "flow_pair"): dict(npts, corners (npts, 2), next_pts (npts, 2), status,
        state, F (3, 3), nf).  F holds findFundamentalMat's result only where the pair's T_M is
        not None.  Raises CoebError when the context holds no batch or z is out of range."""
        r = self.debug_read("flow_pair", z).view(FLOW_PAIR_DTYPE)[0]
        n = max(0, min(int(r["npts"]), FLOW_PAIR_PTS))
        return dict(npts=int(r["npts"]), corners=r["pts"][:n].copy(), next_pts=r["nxt"][:n].copy(),
                    status=r["status"][:n].copy(), state=r["state"][:n].copy(), F=r["F"].reshape(3, 3).copy(),
                    nf=int(r["nf"]))

    # ---- caller-owned device buffers ----
    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        buf = DeviceBuffer(self, arr.nbytes)
        buf.write(arr)
        return buf

    def download(self, dptr, nbytes, dtype=np.uint8):
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype)
        if nbytes:
            self.check(lib().coeb_memcpy_d2h(self.h, _p(out), C.c_void_p(dptr), nbytes))
        return out

    def download_into(self, dptr, out):
        """Copy out.nbytes bytes from device pointer dptr into the contiguous array out."""
        assert out.flags["C_CONTIGUOUS"]
        if out.nbytes:
            self.check(lib().coeb_memcpy_d2h(self.h, _p(out), C.c_void_p(dptr), out.nbytes))
        return out

    # ---- profiling (HIP events on the context stream) ----
    def profile(self, enable=True):
        self.check(lib().coeb_profile_enable(self.h, int(enable)))

    def profile_reset(self):
        self.check(lib().coeb_profile_reset(self.h))

    def profile_read(self):
        names = C.create_string_buffer(4096)
        ms = np.zeros(64, np.float64)
        cnt = np.zeros(64, np.int64)
        nk = C.c_int()
        self.check(lib().coeb_profile_read(self.h, names, 4096, _p(ms), _p(cnt), 64, C.byref(nk)))
        nm = names.value.decode().split(",") if nk.value else []
        return {nm[i]: (float(ms[i]), int(cnt[i])) for i in range(nk.value)}


class DeviceBuffer:
    """hipMalloc'ed buffer on the context's device (torch.cuda is not used in-process: the
    torch wheel bundles its own HIP/HSA runtime, which cannot share a process with the
    system ROCm runtime libcoeb_front.so links)."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        ctx.check(lib().coeb_device_alloc(ctx.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def write(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        self.ctx.check(lib().coeb_memcpy_h2d(self.ctx.h, C.c_void_p(self.ptr + offset), _p(arr), arr.nbytes))

    def read(self, dtype=np.uint8, count=None, offset=0):
        dt = np.dtype(dtype)
        count = (self.nbytes - offset) // dt.itemsize if count is None else count
        return self.ctx.download(self.ptr + offset, count * dt.itemsize, dt)

    def free(self):
        if self.ptr is not None and self.ctx.h is not None:
            lib().coeb_device_free(self.ctx.h, C.c_void_p(self.ptr))
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HostBuffer:
    """Page-locked host memory (coeb_host_alloc) viewed as a numpy array: copies between it and
    the device run asynchronously on the DMA engines (coeb_memcpy_*_async)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        rc = lib().coeb_host_alloc(self.nbytes, C.byref(p))
        if rc != 0:
            raise CoebError("coeb_host_alloc rc=%d: %s" % (rc, lib().coeb_last_error(None).decode()))
        self.ptr = p.value
        self.array = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self.ptr))

    def view(self, dtype, shape=None):
        a = self.array.view(dtype)
        return a if shape is None else a[:int(np.prod(shape))].reshape(shape)

    def free(self):
        if self.ptr is not None:
            self.array = None
            lib().coeb_host_free(C.c_void_p(self.ptr))
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class RGBDStream:
    """The RGB-D Frame constructor (Frame.cc:157-223) on a stream of frames: one coeb_rgbd_stream.
    frame() takes the image as GrabImageRGBD receives it -- (H, W) gray, (H, W, 3) or (H, W, 4)
    u8, strided rows allowed -- and returns dict(tm, n_tm, blur, gray, kps, kps_un, desc, u_right,
    depth, first): ProcessMovingObject against the previous frame, the blur flag of every box, the
    extraction with both, UndistortKeyPoints and ComputeStereoFromRGBD in one call.  n_tm = -1: the
    fundamental matrix was empty (tm is then empty, the frame extracted without T_M).  shadow=False
    runs the previous-frame-only work inside the next call (COEB_STREAM_NO_SHADOW).  close() before
    the context is closed."""

    def __init__(self, ctx, shadow=True):
        self.ctx = ctx
        h = C.c_void_p()
        ctx.check(lib().coeb_rgbd_stream_create(ctx.h, 0 if shadow else STREAM_NO_SHADOW, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            lib().coeb_rgbd_stream_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self.ctx.check(lib().coeb_rgbd_stream_reset(self.h))

    def frame(self, img, depth, cam, dist=None, boxes=None, depth_scale=1.0, rgb_order=True, want_gray=True):
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim not in (2, 3) or img.strides[1] != (1 if img.ndim == 2 else img.shape[2]) or \
                (img.ndim == 3 and img.strides[2] != 1):
            img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape[:2]
        ch = 1 if img.ndim == 2 else img.shape[2]
        depth = np.asarray(depth)
        if depth.shape != (h, w) or depth.dtype not in (np.uint16, np.float32):
            raise ValueError("depth must be (H, W) uint16 or float32")
        if depth.strides[1] != depth.itemsize:
            depth = np.ascontiguousarray(depth)
        dtype = DEPTH_F32 if depth.dtype == np.float32 else DEPTH_U16
        d = None
        if dist is not None:
            d = np.zeros(5, np.float32)
            d[:len(dist)] = np.asarray(dist, np.float32)
        boxes = None if boxes is None else np.ascontiguousarray(boxes, np.float32)
        nb = 0 if boxes is None else len(boxes)
        cap = self.ctx.max_keypoints(w, h)
        kps, kun = np.empty(cap, KEYPOINT_DTYPE), np.empty(cap, KEYPOINT_DTYPE)
        desc = np.empty((cap, 32), np.uint8)
        ur, dep = np.empty(cap, np.float32), np.empty(cap, np.float32)
        tm = np.empty((STREAM_TM_CAP, 2), np.float32)
        blur = np.empty(max(nb, 1), np.int32)
        gray = np.empty((h, w), np.uint8) if want_gray else None
        o = RgbdStreamOutC(_p(tm), STREAM_TM_CAP, 0, _p(blur), _p(gray), w, _p(kps), _p(kun), _p(desc), _p(ur), _p(dep),
                           cap, 0, 0)
        self.ctx.check(lib().coeb_rgbd_stream_frame(self.h, _p(img), img.strides[0], ch, 1 if rgb_order else 0, w, h,
                                                    _p(depth), depth.strides[0], dtype, C.c_float(depth_scale),
                                                    C.byref(cam), _p(d), _p(boxes) if nb else None, nb, C.byref(o)))
        n = o.n
        return dict(tm=tm[:max(o.n_tm, 0)], n_tm=o.n_tm, blur=blur[:nb], gray=gray, kps=kps[:n], kps_un=kun[:n],
                    desc=(desc[:n] if n else None), u_right=ur[:n], depth=dep[:n], first=bool(o.first))


def UndistortKeyPoints(ctx, keys, camera, dist):
    """Frame::UndistortKeyPoints (Frame.cc:579-609): mvKeysUn from mvKeys; dist = mDistCoef
    (k1, k2, p1, p2[, k3])."""
    keys = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
    d = np.zeros(5, np.float32)
    d[:len(dist)] = np.asarray(dist, np.float32)
    out = keys.copy()
    ctx.check(lib().coeb_undistort_keypoints(ctx.h, C.byref(camera), _p(d), _p(keys), len(keys), _p(out)))
    return out


def GrabImageRGBD(ctx, imRGB, imD=None, mbRGB=True, mDepthMapFactor=1.0):
    """The input conversions of Tracking::GrabImageRGBD (src/Tracking.cc:212-228) on the device:
    imRGB (H, W) gray, (H, W, 3) RGB/BGR or (H, W, 4) RGBA/BGRA u8 -> gray u8; imD (H, W) uint16
    or float32 -> float32 via convertTo(CV_32F, mDepthMapFactor) (a float32 map with factor 1 is
    kept as is).  mDepthMapFactor is the Tracking member, i.e. 1 / DepthMapFactor of the YAML.
    Returns (gray, depth or None)."""
    img = np.ascontiguousarray(imRGB, np.uint8)
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    gray = np.empty((h, w), np.uint8)
    dep, dtype, dstride = None, 0, 0
    if imD is not None:
        d = np.ascontiguousarray(imD)
        if d.shape != (h, w) or d.dtype not in (np.uint16, np.float32):
            raise ValueError("imD must be (H, W) uint16 or float32")
        dtype = 1 if d.dtype == np.float32 else 0
        dstride = d.strides[0]
        dep = np.empty((h, w), np.float32)
    ctx.check(lib().coeb_rgbd_preprocess(ctx.h, _p(img), ch * w, ch, 1 if mbRGB else 0,
                                         _p(d) if imD is not None else None, dstride, dtype,
                                         C.c_float(mDepthMapFactor), w, h, _p(gray), _p(dep)))
    return gray, dep


def tum_read_file_list(text_or_path):
    """associate.py read_file_list (associate.py:49-69) through coeb_tum_read_list: a dict
    {stamp: [data fields]} of a TUM list file (a path, or the file's text if it holds a newline)."""
    if "\n" not in text_or_path:
        with open(text_or_path) as f:
            text_or_path = f.read()
    raw = text_or_path.encode()
    cap = raw.count(b"\n") + 1
    st = np.zeros(cap, np.float64)
    off = np.zeros(cap, np.int64)
    ln = np.zeros(cap, np.int32)
    n = C.c_int(0)
    rc = lib().coeb_tum_read_list(raw, len(raw), _p(st), _p(off), _p(ln), cap, C.byref(n))
    if rc != 0:
        raise CoebError("coeb_tum_read_list: %d (a stamp field is not a float literal)" % rc)
    sep = re.compile(r"[ ,\t]+")
    return {float(st[i]): [v.strip() for v in sep.split(raw[off[i]:off[i] + ln[i]].decode()) if v.strip()]
            for i in range(n.value)}


def tum_associate(first, second, offset=0.0, max_difference=0.02):
    """associate.py associate (associate.py:71-102) through coeb_tum_associate: the matched
    (stamp_first, stamp_second) pairs ordered by stamp.  first / second: stamp collections (the
    dicts of tum_read_file_list, or arrays)."""
    a = np.ascontiguousarray(list(first), np.float64)
    b = np.ascontiguousarray(list(second), np.float64)
    cap = max(1, min(len(a), len(b)))
    ia = np.zeros(cap, np.int32)
    ib = np.zeros(cap, np.int32)
    n = C.c_int(0)
    rc = lib().coeb_tum_associate(_p(a), len(a), _p(b), len(b), float(offset), float(max_difference), _p(ia), _p(ib),
                                  cap, C.byref(n))
    if rc != 0:
        raise CoebError("coeb_tum_associate: %d" % rc)
    return [(float(a[ia[k]]), float(b[ib[k]])) for k in range(n.value)]


def boxes_from_ros(xyxy):
    """yolov5_ros_msgs/BoundingBoxes (int64 xmin, ymin, xmax, ymax rows) -> float32 [n, 4] as
    ros_rgbd.cc:106-115 builds them."""
    a = np.ascontiguousarray(np.asarray(xyxy, np.int64).reshape(-1, 4))
    out = np.zeros((len(a), 4), np.float32)
    if len(a) and lib().coeb_boxes_from_int64(_p(a), len(a), _p(out)) != 0:
        raise CoebError("coeb_boxes_from_int64 failed")
    return out


class ORBextractor:
    """Drop-in mirror of ORB_SLAM2::ORBextractor (include/ORBextractor.h:44-128)."""

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device=0, max_width=1280,
                 max_height=960):
        self.ctx = Context(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device, max_width, max_height, 1)
        t = self.ctx.tables()
        self.nlevels = nlevels
        self.scaleFactor = scaleFactor
        self.mvScaleFactor = list(t.scale[:nlevels])
        self.mvInvScaleFactor = list(t.inv_scale[:nlevels])
        self.mvLevelSigma2 = list(t.sigma2[:nlevels])
        self.mvInvLevelSigma2 = list(t.inv_sigma2[:nlevels])
        self.mnFeaturesPerLevel = list(t.features_per_level[:nlevels])
        self.umax = list(t.umax)

    def __call__(self, image, mask=None, img=None, imD=None, box=None, T_M=None, mask_result=None, blur_flag=None):
        """operator()(image, mask, img, imD, keypoints, descriptors, box, T_M, mask_result, blur_flag).
        mask, img, imD and mask_result are accepted and ignored, as in the reference."""
        image = np.asarray(image)
        if image.size == 0:
            return np.zeros(0, KEYPOINT_DTYPE), None
        assert image.dtype == np.uint8 and image.ndim == 2, "image.type() == CV_8UC1 (ORBextractor.cc:1099)"
        boxes = None if not box else np.asarray(box, np.float32).reshape(-1, 4)
        tm = None if T_M is None or len(T_M) == 0 else np.asarray(T_M, np.float32).reshape(-1, 2)
        bf = None if blur_flag is None or len(blur_flag) == 0 else np.asarray(blur_flag, np.int32)
        return self.ctx.extract(image, boxes, tm, bf)

    def GetLevels(self):
        return self.nlevels

    def GetScaleFactor(self):
        return self.scaleFactor

    def GetScaleFactors(self):
        return list(self.mvScaleFactor)

    def GetInverseScaleFactors(self):
        return list(self.mvInvScaleFactor)

    def GetScaleSigmaSquares(self):
        return list(self.mvLevelSigma2)

    def GetInverseScaleSigmaSquares(self):
        return list(self.mvInvLevelSigma2)


class Frame:
    """The Frame fields SearchByProjection reads (src/Frame.cc / include/Frame.h)."""

    def __init__(self, keys_un, descriptors, u_right=None, Tcw=None, map_points=None, outlier=None):
        self.mvKeysUn = np.ascontiguousarray(keys_un)
        self.N = len(self.mvKeysUn)
        self.mDescriptors = np.ascontiguousarray(descriptors, np.uint8).reshape(self.N, 32) if self.N else \
            np.zeros((0, 32), np.uint8)
        self.mvuRight = np.full(self.N, -1, np.float32) if u_right is None else np.ascontiguousarray(u_right, np.float32)
        self.mTcw = np.eye(4, dtype=np.float32) if Tcw is None else np.ascontiguousarray(Tcw, np.float32)
        # map_points: dict(world_pos [N,3] f32, descriptor [N,32] u8, observations [N] i32, valid [N] u8)
        self.map_points = map_points
        self._outlier = None if outlier is None else np.ascontiguousarray(outlier, np.uint8)
        self.mvpMapPoints = np.full(self.N, -1, np.int32)
        self._mp_obs = None
        self._mp_pos = None

    # the fields below are allocated on first use (a per-frame cost of the Python binding the
    # drop-in latency in bench.py includes; the C++ Tracking thread owns them already)
    def ComputeBoW(self, ctx, levelsup=4):
        """Frame::ComputeBoW (Frame.cc:570-577) with the context's vocabulary: mBowWord / mBowWeight
        per feature (mBowVec's entries before the caller's normalisation), mFeatNode (the
        FeatureVector node of each feature, -1: none) and mFeatVec as (node ids, offsets, indices)."""
        r = ctx.bow_transform(self.mDescriptors, levelsup)
        self.mBowWord, self.mBowWeight, self.mFeatNode = r["word"], r["weight"], r["node"]
        self.mFeatVec = (r["fv_node"], r["fv_off"], r["fv_idx"])

    @property
    def mvbOutlier(self):
        if self._outlier is None:
            self._outlier = np.zeros(self.N, np.uint8)
        return self._outlier

    @mvbOutlier.setter
    def mvbOutlier(self, v):
        self._outlier = v

    @property
    def mvpMapPointObs(self):
        """Observations() of the MapPoint in mvpMapPoints[i] (-1 = NULL); read by the local-map search."""
        if self._mp_obs is None:
            self._mp_obs = np.full(self.N, -1, np.int32)
        return self._mp_obs

    @mvpMapPointObs.setter
    def mvpMapPointObs(self, v):
        self._mp_obs = v

    @property
    def mvMapPointPos(self):
        """GetWorldPos() of the MapPoint in mvpMapPoints[i]; read by Optimizer.PoseOptimization."""
        if self._mp_pos is None:
            self._mp_pos = np.zeros((self.N, 3), np.float32)
        return self._mp_pos

    @mvMapPointPos.setter
    def mvMapPointPos(self, v):
        self._mp_pos = v


class LocalMap:
    """vpLocalMapPoints after Tracking::SearchLocalPoints ran Frame::isInFrustum on them
    (src/Tracking.cc:1244-1259, src/Frame.cc:445-501): the fields ORBmatcher::SearchByProjection(F, vpMapPoints, th) reads (ORBmatcher.cc:50-80)."""

    def __init__(self, in_view, proj_x, proj_y, proj_xr, level, view_cos, descriptor, observations):
        self.mbTrackInView = np.ascontiguousarray(in_view, np.uint8)
        self.N = len(self.mbTrackInView)
        self.mTrackProjX = np.ascontiguousarray(proj_x, np.float32)
        self.mTrackProjY = np.ascontiguousarray(proj_y, np.float32)
        self.mTrackProjXR = np.ascontiguousarray(proj_xr, np.float32)
        self.mnTrackScaleLevel = np.ascontiguousarray(level, np.int32)
        self.mTrackViewCos = np.ascontiguousarray(view_cos, np.float32)
        self.mDescriptor = np.ascontiguousarray(descriptor, np.uint8).reshape(self.N, 32) if self.N else \
            np.zeros((0, 32), np.uint8)
        self.nObs = np.ascontiguousarray(observations, np.int32)
        for a in (self.mTrackProjX, self.mTrackProjY, self.mTrackProjXR, self.mnTrackScaleLevel, self.mTrackViewCos,
                  self.nObs):
            if len(a) != self.N:
                raise ValueError("LocalMap arrays differ in length")

    def c_struct(self):
        return LocalMapC(self.N, *[C.c_void_p(a.ctypes.data) for a in (
            self.mbTrackInView, self.mTrackProjX, self.mTrackProjY, self.mTrackProjXR, self.mnTrackScaleLevel,
            self.mTrackViewCos, self.mDescriptor, self.nObs)])


class LocalPoints:
    """vpLocalMapPoints as Tracking::SearchLocalPoints reads them before isInFrustum
    (src/Tracking.cc:1246-1259): per point, valid (!isBad() and not seen in this frame),
    GetWorldPos(), GetNormal(), mfMaxDistance, mfMinDistance, GetDescriptor() and Observations()."""

    def __init__(self, valid, world_pos, normal, max_distance, min_distance, descriptor, observations):
        self.valid = np.ascontiguousarray(valid, np.uint8)
        self.N = len(self.valid)
        self.world_pos = np.ascontiguousarray(world_pos, np.float32).reshape(self.N, 3)
        self.normal = np.ascontiguousarray(normal, np.float32).reshape(self.N, 3)
        self.max_distance = np.ascontiguousarray(max_distance, np.float32)
        self.min_distance = np.ascontiguousarray(min_distance, np.float32)
        self.descriptor = np.ascontiguousarray(descriptor, np.uint8).reshape(self.N, 32) if self.N else \
            np.zeros((0, 32), np.uint8)
        self.observations = np.ascontiguousarray(observations, np.int32)
        for a in (self.max_distance, self.min_distance, self.observations):
            if len(a) != self.N:
                raise ValueError("LocalPoints arrays differ in length")

    def c_struct(self):
        return LocalPointsC(self.N, *[C.c_void_p(a.ctypes.data) for a in (
            self.valid, self.world_pos, self.normal, self.max_distance, self.min_distance, self.descriptor,
            self.observations)])


TRACK_FIELDS = (("in_view", np.uint8), ("proj_x", np.float32), ("proj_y", np.float32), ("proj_xr", np.float32),
                ("level", np.int32), ("view_cos", np.float32))


def _track_fields(n):
    arrs = {k: np.zeros(max(n, 1), dt) for k, dt in TRACK_FIELDS}
    return arrs, TrackFieldsC(*[C.c_void_p(arrs[k].ctypes.data) for k, _ in TRACK_FIELDS])


def search_local_points(ctx, camera, F, cur_observations, points, cos_limit=0.5, th=3.0, nnratio=0.8,
                        track_fields=True):
    """Tracking::SearchLocalPoints from the projection loop on (src/Tracking.cc:1246-1271) in one
    call (coeb_search_local_points): isInFrustum(pMP, cos_limit) with F.mTcw over `points` (a
    LocalPoints), then SearchByProjection(F, vpLocalMapPoints, th).  cur_observations: i32[F.N]
    Observations() of the MapPoint each keypoint holds (-1: none), or None.  Returns a dict:
    the six TRACK_FIELDS arrays (when track_fields), match (i32[F.N], local-map index or -1),
    n_to_match, nmatches."""
    cf = CurFrameC(F.N, C.c_void_p(F.mvKeysUn.ctypes.data), C.c_void_p(F.mDescriptors.ctypes.data),
                   C.c_void_p(F.mvuRight.ctypes.data))
    cobs = None if cur_observations is None else np.ascontiguousarray(cur_observations, np.int32)
    T = np.ascontiguousarray(F.mTcw, np.float32)
    lp = points.c_struct()
    arrs, tf = _track_fields(points.N) if track_fields else ({}, None)
    match = np.full(max(F.N, 1), -1, np.int32)
    ntm, nm = C.c_int(), C.c_int()
    ctx.check(lib().coeb_search_local_points(ctx.h, C.byref(camera), C.byref(cf), _p(cobs), _p(T), C.byref(lp),
                                             cos_limit, th, nnratio, C.byref(tf) if tf is not None else None,
                                             _p(match), C.byref(ntm), C.byref(nm)))
    res = {k: v[:points.N] for k, v in arrs.items()}
    res.update(match=match[:F.N], n_to_match=ntm.value, nmatches=nm.value)
    return res


def track_local_map(ctx, camera, F, cur_observations, cur_world_pos, points, cos_limit=0.5, th=3.0, nnratio=0.8,
                    only_tracking=False, track_fields=True):
    """Tracking::TrackLocalMap after UpdateLocalMap (src/Tracking.cc:996-1047) in one call
    (coeb_track_local_map): search_local_points, Optimizer::PoseOptimization from F.mTcw over the
    keypoints that hold a point afterwards (the search's, else the entry MapPoint:
    cur_observations[i] >= 0 at cur_world_pos[i]) and mnMatchesInliers.  F is not modified.
    Returns a dict: the TRACK_FIELDS arrays (when track_fields), match, n_to_match, nlocal,
    Tcw (4x4 f32), outlier (u8[F.N], 0 where the keypoint holds no point), ninliers_pose,
    nmatches_inliers."""
    cf = CurFrameC(F.N, C.c_void_p(F.mvKeysUn.ctypes.data), C.c_void_p(F.mDescriptors.ctypes.data),
                   C.c_void_p(F.mvuRight.ctypes.data))
    cobs = None if cur_observations is None else np.ascontiguousarray(cur_observations, np.int32)
    cxw = None if cur_world_pos is None else np.ascontiguousarray(cur_world_pos, np.float32)
    T = np.ascontiguousarray(F.mTcw, np.float32).copy()
    lp = points.c_struct()
    arrs, tf = _track_fields(points.N) if track_fields else ({}, None)
    match = np.full(max(F.N, 1), -1, np.int32)
    outl = np.zeros(max(F.N, 1), np.uint8)
    ntm, nl, nin, nmi = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    ctx.check(lib().coeb_track_local_map(ctx.h, C.byref(camera), C.byref(cf), _p(cobs), _p(cxw), _p(T), C.byref(lp),
                                         cos_limit, th, nnratio, int(bool(only_tracking)),
                                         C.byref(tf) if tf is not None else None, _p(match), _p(outl), C.byref(ntm),
                                         C.byref(nl), C.byref(nin), C.byref(nmi)))
    res = {k: v[:points.N] for k, v in arrs.items()}
    res.update(match=match[:F.N], n_to_match=ntm.value, nlocal=nl.value, Tcw=T.reshape(4, 4), outlier=outl[:F.N],
               ninliers_pose=nin.value, nmatches_inliers=nmi.value)
    return res


class KeyFramePoints:
    """pKF->GetMapPointMatches() snapshot for the relocalisation search (ORBmatcher.cc:1487-1530):
    per slot i, valid (pMP && !isBad()), GetWorldPos(), GetDescriptor(), mfMaxDistance,
    mfMinDistance and pKF->mvKeysUn[i].angle.  sAlreadyFound is passed to SearchByProjection as
    a set of slot indices."""

    def __init__(self, valid, world_pos, descriptor, max_distance, min_distance, angle):
        self.valid = np.ascontiguousarray(valid, np.uint8)
        self.N = len(self.valid)
        self.world_pos = np.ascontiguousarray(world_pos, np.float32).reshape(self.N, 3)
        self.descriptor = np.ascontiguousarray(descriptor, np.uint8).reshape(self.N, 32) if self.N else \
            np.zeros((0, 32), np.uint8)
        self.max_distance = np.ascontiguousarray(max_distance, np.float32)
        self.min_distance = np.ascontiguousarray(min_distance, np.float32)
        self.angle = np.ascontiguousarray(angle, np.float32)
        for a in (self.max_distance, self.min_distance, self.angle):
            if len(a) != self.N:
                raise ValueError("KeyFramePoints arrays differ in length")


class BowKeyFrame:
    """The KeyFrame fields SearchByBoW reads (ORBmatcher.cc:161-199, 234): per feature i, valid
    (GetMapPointMatches()[i] && !isBad()), mDescriptors.row(i), the mFeatVec node that lists it
    (-1: none) and mvKeysUn[i].angle."""

    def __init__(self, valid, descriptor, node_id, angle):
        self.valid = np.ascontiguousarray(valid, np.uint8)
        self.N = len(self.valid)
        self.descriptor = np.ascontiguousarray(descriptor, np.uint8).reshape(self.N, 32) if self.N else \
            np.zeros((0, 32), np.uint8)
        self.node_id = np.ascontiguousarray(node_id, np.int32)
        self.angle = np.ascontiguousarray(angle, np.float32)
        if len(self.node_id) != self.N or len(self.angle) != self.N:
            raise ValueError("BowKeyFrame arrays differ in length")


def bow_vector(word, weight, node, normalize_l1=True):
    """DBoW2::BowVector of one frame from coeb_bow_transform's per-feature word / weight / node:
    addWeight in feature order over the features with node >= 0, then normalize(L1) (host only).
    -> (word ids ascending int32, values float64)."""
    word = np.ascontiguousarray(word, np.int32)
    weight = np.ascontiguousarray(weight, np.float64)
    node = np.ascontiguousarray(node, np.int32)
    n = len(word)
    if len(weight) != n or len(node) != n:
        raise ValueError("bow_vector arrays differ in length")
    w_out, v_out = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.float64)
    nw = C.c_int()
    rc = lib().coeb_bow_vector(_p(word), _p(weight), _p(node), n, int(bool(normalize_l1)), _p(w_out), _p(v_out), n,
                               C.byref(nw))
    if rc:
        raise CoebError("coeb_bow_vector rc=%d" % rc)
    return w_out[:nw.value].copy(), v_out[:nw.value].copy()


# coeb_kf_view: one keyframe as CreateNewMapPoints' loop reads it
KF_VIEW_DTYPE = np.dtype([("Rcw", np.float32, (9,)), ("tcw", np.float32, (3,)), ("Ow", np.float32, (3,)),
                          ("fx", np.float32), ("fy", np.float32), ("cx", np.float32), ("cy", np.float32),
                          ("invfx", np.float32), ("invfy", np.float32), ("mb", np.float32), ("mbf", np.float32)])
NEWPTS_NO_PAIR, NEWPTS_ACCEPTED, NEWPTS_LOW_PARALLAX, NEWPTS_W_ZERO, NEWPTS_Z1, NEWPTS_Z2, NEWPTS_REPROJ1, \
    NEWPTS_REPROJ2, NEWPTS_ZERO_DIST, NEWPTS_RATIO = range(10)
NEWPTS_SRC_TRIANGULATED, NEWPTS_SRC_STEREO1, NEWPTS_SRC_STEREO2 = 1, 2, 3


def kf_view(Rcw, tcw, Ow, fx, fy, cx, cy, invfx, invfy, mb, mbf):
    """One KF_VIEW_DTYPE record; every entry is the caller's (nothing is derived)."""
    v = np.zeros((), KF_VIEW_DTYPE)
    v["Rcw"], v["tcw"], v["Ow"] = np.asarray(Rcw, np.float32).reshape(9), np.asarray(tcw, np.float32).reshape(3), \
        np.asarray(Ow, np.float32).reshape(3)
    for k, x in zip(("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf"), (fx, fy, cx, cy, invfx, invfy, mb, mbf)):
        v[k] = x
    return v


class KeyFrameDatabase:
    """ORB_SLAM2::KeyFrameDatabase for relocalisation, device resident (include/KeyFrameDatabase.h,
    src/KeyFrameDatabase.cc:40-73, 199-309): a keyframe's descriptors, feature-vector nodes, angles
    and BowVector are uploaded once by add(); query() counts common words and scores against every
    keyframe in one call; SearchByBoW() matches a frame against many keyframes in one call.
    Keyframes are named by the slot add() returns.  The scoring restates DBoW2's L1Scoring; parity
    against DBoW2 itself is unpinned."""

    def __init__(self, ctx, max_features=4095, initial_slots=64):
        self.ctx = ctx
        h = C.c_void_p()
        ctx.check(lib().coeb_kfdb_create(ctx.h, max_features, initial_slots, C.byref(h)))
        self.h = h
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = {}, {}, {}
        self._query_id = 0
        self._n = {}                    # features per slot

    def close(self):
        if getattr(self, "h", None):
            lib().coeb_kfdb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if getattr(self.ctx, "h", None):       # a closed context has released the storage already
                self.close()
        except Exception:
            pass

    def add(self, descriptor, node_id, angle, bow_word, bow_value):
        """KeyFrameDatabase::add(pKF) -> slot.  bow_word strictly ascending (bow_vector())."""
        node_id = np.ascontiguousarray(node_id, np.int32)
        n = len(node_id)
        descriptor = np.ascontiguousarray(descriptor, np.uint8).reshape(n, 32) if n else np.zeros((0, 32), np.uint8)
        angle = np.ascontiguousarray(angle, np.float32)
        bow_word = np.ascontiguousarray(bow_word, np.int32)
        bow_value = np.ascontiguousarray(bow_value, np.float64)
        if len(angle) != n or len(bow_value) != len(bow_word):
            raise ValueError("KeyFrameDatabase.add arrays differ in length")
        kc = KfdbKeyFrameC(n, _p(descriptor), _p(node_id), _p(angle), _p(bow_word), _p(bow_value), len(bow_word))
        slot = C.c_int()
        self.ctx.check(lib().coeb_kfdb_add(self.h, C.byref(kc), C.byref(slot)))
        for d in (self.mnRelocQuery, self.mnRelocWords, self.mRelocScore):
            d.pop(slot.value, None)
        self._n[slot.value] = n
        return slot.value

    def erase(self, slot):
        self.ctx.check(lib().coeb_kfdb_erase(self.h, int(slot)))

    def clear(self):
        self.ctx.check(lib().coeb_kfdb_clear(self.h))
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = {}, {}, {}

    def size(self):
        """(keyframes, slots: the length of query()'s arrays)"""
        nk, ns = C.c_int(), C.c_int()
        self.ctx.check(lib().coeb_kfdb_size(self.h, C.byref(nk), C.byref(ns)))
        return nk.value, ns.value

    def query(self, word, value):
        """The query BowVector against every keyframe: dict(common [nslots] = mnRelocWords,
        score [nslots] float32 (-1 where common <= min_common), order = lKFsSharingWords as slots,
        max_common, min_common)."""
        word = np.ascontiguousarray(word, np.int32)
        value = np.ascontiguousarray(value, np.float64)
        if len(word) != len(value):
            raise ValueError("query arrays differ in length")
        ns = self.size()[1]
        common, score, order = np.zeros(max(ns, 1), np.int32), np.zeros(max(ns, 1), np.float32), \
            np.zeros(max(ns, 1), np.int32)
        nsh, mx, mn = C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(lib().coeb_kfdb_query(self.h, _p(word), _p(value), len(word), _p(common), _p(score), _p(order),
                                             C.byref(nsh), C.byref(mx), C.byref(mn)))
        return dict(common=common[:ns], score=score[:ns], order=order[:nsh.value].copy(), max_common=mx.value,
                    min_common=mn.value)

    def DetectRelocalizationCandidates(self, F, neighbours=None):
        """KeyFrameDatabase::DetectRelocalizationCandidates(F) -> candidate slots.  F: a Frame after
        ComputeBoW (F.mBowVec = (word, value) is filled from it when absent); F.mnId names the query
        (a fresh id when absent).  neighbours(slot) -> the slots of GetBestCovisibilityKeyFrames(10);
        the covisibility tail (:258-308) runs here on the host."""
        if getattr(F, "mBowVec", None) is None:
            F.mBowVec = bow_vector(F.mBowWord, F.mBowWeight, F.mFeatNode)
        self._query_id += 1
        fid = getattr(F, "mnId", ("query", self._query_id))
        q = self.query(*F.mBowVec)
        for s in q["order"]:
            self.mnRelocQuery[int(s)] = fid
            self.mnRelocWords[int(s)] = int(q["common"][s])
        scored = [int(s) for s in q["order"] if q["common"][s] > q["min_common"]]
        for s in scored:
            self.mRelocScore[s] = q["score"][s]
        acc, best_acc = [], np.float32(0)
        for s in scored:
            best_score = acc_score = q["score"][s]
            best = s
            for s2 in (neighbours(s) if neighbours else ()):
                if self.mnRelocQuery.get(s2) != fid:
                    continue
                sc2 = np.float32(self.mRelocScore.get(s2, 0.0))
                acc_score = np.float32(acc_score + sc2)
                if sc2 > best_score:
                    best, best_score = s2, sc2
            acc.append((acc_score, best))
            if acc_score > best_acc:
                best_acc = acc_score
        min_retain = np.float32(0.75) * best_acc
        out = []
        for si, s in acc:
            if si > min_retain and s not in out:
                out.append(s)
        return out

    def SearchByBoW(self, slots, valids, F, nnratio=0.75, checkOri=True):
        """ORBmatcher(nnratio, checkOri).SearchByBoW(pKF, F, vpMapPointMatches) for every candidate
        slot (Tracking.cc:1449-1470); valids[j]: GetMapPointMatches()[i] && !isBad() of candidate j.
        -> (matches [ncand][F.N]: the keyframe feature whose MapPoint keypoint i takes or -1,
        nmatches [ncand])."""
        slots = np.ascontiguousarray(slots, np.int32)
        nc = len(slots)
        if len(valids) != nc:
            raise ValueError("one valid mask per candidate")
        valids = [np.ascontiguousarray(v, np.uint8) for v in valids]
        for s, v in zip(slots, valids):
            if int(s) in self._n and len(v) != self._n[int(s)]:
                raise ValueError("valid mask of slot %d has %d entries, the keyframe %d" % (s, len(v), self._n[int(s)]))
        vp = (C.c_void_p * max(nc, 1))(*[v.ctypes.data if len(v) else None for v in valids])
        node = np.ascontiguousarray(F.mFeatNode, np.int32)
        angle = np.ascontiguousarray(F.mvKeysUn["angle"], np.float32)
        fc = BowFrameC(F.N, *[C.c_void_p(a.ctypes.data) for a in (F.mDescriptors, node, angle)])
        out = np.full((nc, F.N), -1, np.int32)
        nm = np.zeros(max(nc, 1), np.int32)
        self.ctx.check(lib().coeb_match_bow_kfdb(self.h, _p(slots) if nc else None, nc, vp, C.byref(fc), nnratio,
                                                 int(checkOri), _p(out) if out.size else None, _p(nm)))
        return out, nm[:nc]

    def set_geometry(self, slot, keys_un, u_right):
        """What SearchForTriangulation reads of the keyframe in `slot` beyond add()'s arrays: mvKeysUn
        (pt, octave) and mvuRight, one entry per feature.  erase, clear and the reuse of a slot drop it."""
        keys_un = np.ascontiguousarray(keys_un, KEYPOINT_DTYPE)
        u_right = np.ascontiguousarray(u_right, np.float32)
        n = self._n.get(int(slot))
        if n is not None and (len(keys_un) != n or len(u_right) != n):
            raise ValueError("the keyframe of slot %d has %d features" % (slot, n))
        self.ctx.check(lib().coeb_kfdb_set_geometry(self.h, int(slot), _p(keys_un) if len(keys_un) else None,
                                                    _p(u_right) if len(u_right) else None))

    def search_for_triangulation(self, slot1, has_mp1, slots2, has_mp2, F12, epipole, only_stereo, check_orientation):
        """ORBmatcher(_, check_orientation).SearchForTriangulation(KF[slot1], KF[slots2[j]], F12[j], .., only_stereo)
        for every neighbour j in one call (LocalMapping::CreateNewMapPoints).  has_mp1 / has_mp2[j]:
        GetMapPoint(i) != NULL per feature; F12 [nnb, 3, 3] and epipole [nnb, 2] = (ex, ey) are the caller's.
        -> (match [nnb, n1] int32: vMatches12, nmatches [nnb])."""
        slots2 = np.ascontiguousarray(slots2, np.int32)
        nnb = len(slots2)
        if len(has_mp2) != nnb:
            raise ValueError("one has_mp2 mask per neighbour")
        has_mp1 = np.ascontiguousarray(has_mp1, np.uint8)
        has_mp2 = [np.ascontiguousarray(m, np.uint8) for m in has_mp2]
        n1 = self._n.get(int(slot1), len(has_mp1))
        if len(has_mp1) != n1:
            raise ValueError("has_mp1 has %d entries, the keyframe %d" % (len(has_mp1), n1))
        for s, m in zip(slots2, has_mp2):
            if int(s) in self._n and len(m) != self._n[int(s)]:
                raise ValueError("has_mp2 of slot %d has %d entries, the keyframe %d" % (s, len(m), self._n[int(s)]))
        F12 = np.ascontiguousarray(F12, np.float32).reshape(nnb, 9)
        epipole = np.ascontiguousarray(epipole, np.float32).reshape(nnb, 2)
        mp = (C.c_void_p * max(nnb, 1))(*[m.ctypes.data if len(m) else None for m in has_mp2])
        out = np.full((nnb, n1), -1, np.int32)
        nm = np.zeros(max(nnb, 1), np.int32)
        self.ctx.check(lib().coeb_kfdb_search_triangulation(
            self.h, int(slot1), _p(has_mp1) if n1 else None, _p(slots2) if nnb else None, nnb, mp,
            _p(F12) if nnb else None, _p(epipole) if nnb else None, int(bool(only_stereo)), int(bool(check_orientation)),
            _p(out) if out.size else None, _p(nm)))
        return out, nm[:nnb]

    def set_stereo(self, slot, key_xy, depth):
        """What CreateNewMapPoints' triangulation reads of the keyframe in `slot` beyond set_geometry(): the raw
        mvKeys[i].pt [n, 2] and mvDepth [n].  erase, clear and the reuse of a slot drop it."""
        key_xy = np.ascontiguousarray(key_xy, np.float32).reshape(-1, 2)
        depth = np.ascontiguousarray(depth, np.float32)
        n = self._n.get(int(slot))
        if n is not None and (len(key_xy) != n or len(depth) != n):
            raise ValueError("the keyframe of slot %d has %d features" % (slot, n))
        self.ctx.check(lib().coeb_kfdb_set_stereo(self.h, int(slot), _p(key_xy) if len(key_xy) else None,
                                                  _p(depth) if len(depth) else None))

    def create_new_map_points(self, slot1, view1, has_mp1, slots2, views2, has_mp2, F12, epipole, only_stereo=False):
        """LocalMapping::CreateNewMapPoints' search and loop body (LocalMapping.cc:269-433) for every neighbour in
        one call.  view1 / views2[j]: KF_VIEW_DTYPE records (or what kf_view() takes); the other arguments are
        search_for_triangulation's.  -> dict(match [nnb, n1] int32, status [nnb, n1] int8: the way out of the loop
        body (NEWPTS_*), source [nnb, n1] int8: where x3D came from (NEWPTS_SRC_*), x3d [nnb, n1, 3] float32 (NaN
        where the pair was not accepted), first_ok [n1] int32: the neighbour whose pair becomes the MapPoint,
        nmatches [nnb])."""
        slots2 = np.ascontiguousarray(slots2, np.int32)
        nnb = len(slots2)
        if len(has_mp2) != nnb:
            raise ValueError("one has_mp2 mask per neighbour")
        has_mp1 = np.ascontiguousarray(has_mp1, np.uint8)
        has_mp2 = [np.ascontiguousarray(m, np.uint8) for m in has_mp2]
        n1 = self._n.get(int(slot1), len(has_mp1))
        if len(has_mp1) != n1:
            raise ValueError("has_mp1 has %d entries, the keyframe %d" % (len(has_mp1), n1))
        for s, m in zip(slots2, has_mp2):
            if int(s) in self._n and len(m) != self._n[int(s)]:
                raise ValueError("has_mp2 of slot %d has %d entries, the keyframe %d" % (s, len(m), self._n[int(s)]))
        v1 = np.ascontiguousarray(view1, KF_VIEW_DTYPE).reshape(1)
        v2 = np.ascontiguousarray(views2, KF_VIEW_DTYPE).reshape(-1)
        if len(v2) != nnb:
            raise ValueError("one view per neighbour")
        F12 = np.ascontiguousarray(F12, np.float32).reshape(nnb, 9)
        epipole = np.ascontiguousarray(epipole, np.float32).reshape(nnb, 2)
        mp = (C.c_void_p * max(nnb, 1))(*[m.ctypes.data if len(m) else None for m in has_mp2])
        match = np.full((nnb, n1), -1, np.int32)
        status = np.zeros((nnb, n1), np.int8)
        x3d = np.full((nnb, n1, 3), np.nan, np.float32)
        first = np.full(max(n1, 1), -1, np.int32)
        nm = np.zeros(max(nnb, 1), np.int32)
        self.ctx.check(lib().coeb_kfdb_create_new_map_points(
            self.h, int(slot1), _p(v1), _p(has_mp1) if n1 else None, _p(slots2) if nnb else None, nnb,
            _p(v2) if nnb else None, mp, _p(F12) if nnb else None, _p(epipole) if nnb else None, int(bool(only_stereo)),
            _p(match) if match.size else None, _p(status) if match.size else None, _p(x3d) if match.size else None,
            _p(first), _p(nm)))
        return dict(match=match, status=status & 15, source=(status >> 4) & 3, x3d=x3d, first_ok=first[:n1],
                    nmatches=nm[:nnb])

    def fuse_search(self, cam, points, jobs, th=3.0):
        """The search of ORBmatcher::Fuse(KF[slot], vpMapPoints[first : first + count], th) for every job in one
        call (LocalMapping::SearchInNeighbors).  points: dict(valid [n] = pMP && !isBad(), world_pos [n, 3],
        normal [n, 3], max_distance [n] = mfMaxDistance, min_distance [n], descriptor [n, 32]).  jobs: dicts
        (slot, Rcw [3, 3], tcw [3], Ow [3], first = 0, count = to the list's end, skip = None or [count] =
        IsInKeyFrame).  -> (best_idx, best_dist): one int32 array per job; best_idx is bestIdx where bestDist <=
        TH_LOW else -1, best_dist is bestDist (256: no candidate accepted, or the point was skipped or rejected)."""
        valid = np.ascontiguousarray(points["valid"], np.uint8)
        n = len(valid)
        pos = np.ascontiguousarray(points["world_pos"], np.float32).reshape(n, 3)
        nrm = np.ascontiguousarray(points["normal"], np.float32).reshape(n, 3)
        mx = np.ascontiguousarray(points["max_distance"], np.float32)
        mn = np.ascontiguousarray(points["min_distance"], np.float32)
        desc = np.ascontiguousarray(points["descriptor"], np.uint8).reshape(n, 32)
        if len(mx) != n or len(mn) != n:
            raise ValueError("point arrays differ in length")
        pc = FusePointsC(n, *[C.c_void_p(a.ctypes.data) if n else None for a in (valid, pos, nrm, mx, mn, desc)])
        nj = len(jobs)
        jc = (FuseJobC * max(nj, 1))()
        keep, counts = [], []
        for k, j in enumerate(jobs):
            first = int(j.get("first", 0))
            count = int(j["count"]) if j.get("count") is not None else n - first
            jc[k].slot, jc[k].first, jc[k].count = int(j["slot"]), first, count
            jc[k].Rcw[:] = np.asarray(j["Rcw"], np.float32).reshape(9).tolist()
            jc[k].tcw[:] = np.asarray(j["tcw"], np.float32).reshape(3).tolist()
            jc[k].Ow[:] = np.asarray(j["Ow"], np.float32).reshape(3).tolist()
            if j.get("skip") is not None:
                sk = np.ascontiguousarray(j["skip"], np.uint8)
                if len(sk) != count:
                    raise ValueError("skip of job %d has %d entries, its range %d" % (k, len(sk), count))
                keep.append(sk)
                jc[k].skip = sk.ctypes.data if count > 0 else None
            counts.append(count)
        total = sum(c for c in counts if c > 0)
        bi = np.full(max(total, 1), -1, np.int32)
        bd = np.full(max(total, 1), 256, np.int32)
        c = cam if isinstance(cam, Camera) else Camera(*[float(x) for x in cam])
        self.ctx.check(lib().coeb_kfdb_fuse_search(self.h, C.byref(c), C.byref(pc), jc if nj else None, nj, float(th),
                                                   _p(bi) if total else None, _p(bd) if total else None))
        out_i, out_d, o = [], [], 0
        for cnt in counts:
            out_i.append(bi[o:o + cnt].copy())
            out_d.append(bd[o:o + cnt].copy())
            o += cnt
        return out_i, out_d


class ORBmatcher:
    """Mirror of ORB_SLAM2::ORBmatcher for the tracking searches."""
    TH_HIGH = 100
    TH_LOW = 50
    HISTO_LENGTH = 30

    def __init__(self, nnratio=0.6, checkOri=True, ctx=None):
        self.mfNNratio = nnratio
        self.mbCheckOrientation = checkOri
        self.ctx = ctx

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        return lib().coeb_descriptor_distance(_p(a), _p(b))

    def SearchByProjection(self, CurrentFrame, second, *args, **kw):
        """The reference's overloads, by the type of the second argument:
          (CurrentFrame, LastFrame: Frame, th, bMono, camera)        ORBmatcher.cc:1329-1471
          (F, vpMapPoints: LocalMap, th=3, camera=...)                 ORBmatcher.cc:44-129
          (F, pKF: KeyFramePoints, sAlreadyFound, th, ORBdist, camera) ORBmatcher.cc:1473-1600"""
        if self.ctx is None:
            self.ctx = Context()
        if isinstance(second, LocalMap):
            return self._search_local_map(CurrentFrame, second, *args, **kw)
        if isinstance(second, KeyFramePoints):
            return self._search_keyframe(CurrentFrame, second, *args, **kw)
        return self._search_last_frame(CurrentFrame, second, *args, **kw)

    def SearchByBoW(self, pKF, F):
        """SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORBmatcher.cc:159-288): pKF a
        BowKeyFrame, F a Frame after ComputeBoW.  F.mvpMapPoints[i] = the KeyFrame feature whose
        MapPoint keypoint i takes, or -1; returns nmatches."""
        if self.ctx is None:
            self.ctx = Context()
        node = np.ascontiguousarray(F.mFeatNode, np.int32)
        angle = np.ascontiguousarray(F.mvKeysUn["angle"], np.float32)      # mvKeys[i].angle: undistortion keeps it
        kc = BowKeyFrameC(pKF.N, *[C.c_void_p(a.ctypes.data) for a in (pKF.valid, pKF.descriptor, pKF.node_id,
                                                                      pKF.angle)])
        fc = BowFrameC(F.N, *[C.c_void_p(a.ctypes.data) for a in (F.mDescriptors, node, angle)])
        out = np.empty(max(F.N, 1), np.int32)
        nm = C.c_int()
        self.ctx.check(lib().coeb_match_bow(self.ctx.h, C.byref(kc), C.byref(fc), self.mfNNratio,
                                            int(self.mbCheckOrientation), _p(out), C.byref(nm)))
        F.mvpMapPoints = out[:F.N]
        return nm.value

    def _search_last_frame(self, CurrentFrame, LastFrame, th, bMono, camera):
        mp = LastFrame.map_points
        has = np.ascontiguousarray(mp["valid"], np.uint8)
        outl = np.ascontiguousarray(LastFrame.mvbOutlier, np.uint8)
        xw = np.ascontiguousarray(mp["world_pos"], np.float32)
        desc = np.ascontiguousarray(mp["descriptor"], np.uint8)
        nobs = np.ascontiguousarray(mp["observations"], np.int32)
        keys = np.ascontiguousarray(LastFrame.mvKeysUn)
        lf = LastFrameC(LastFrame.N, has.ctypes.data, outl.ctypes.data, xw.ctypes.data, desc.ctypes.data,
                        nobs.ctypes.data, keys.ctypes.data)
        cf = CurFrameC(CurrentFrame.N, CurrentFrame.mvKeysUn.ctypes.data, CurrentFrame.mDescriptors.ctypes.data,
                       CurrentFrame.mvuRight.ctypes.data)
        # every entry of the result is written by the call (matched index or -1)
        out = np.empty(max(CurrentFrame.N, 1), np.int32)
        nm = C.c_int()
        self.ctx.check(lib().coeb_match_lastframe(self.ctx.h, C.byref(camera), C.byref(cf), C.byref(lf),
                                                  _p(CurrentFrame.mTcw), _p(LastFrame.mTcw), th, int(bMono),
                                                  int(self.mbCheckOrientation), _p(out), C.byref(nm)))
        CurrentFrame.mvpMapPoints = out[:CurrentFrame.N]
        return nm.value


    def _search_keyframe(self, F, kf, sAlreadyFound=(), th=10.0, ORBdist=100, camera=None):
        if camera is None:
            raise ValueError("SearchByProjection(F, pKF, sAlreadyFound, th, ORBdist): camera is required")
        valid = kf.valid.copy()
        for i in sAlreadyFound:
            valid[i] = 0
        cf = CurFrameC(F.N, C.c_void_p(F.mvKeysUn.ctypes.data), C.c_void_p(F.mDescriptors.ctypes.data), None)
        has = np.ascontiguousarray(F.mvpMapPoints >= 0, np.uint8)
        kc = KeyFramePointsC(kf.N, *[C.c_void_p(a.ctypes.data) for a in (
            valid, kf.world_pos, kf.descriptor, kf.max_distance, kf.min_distance, kf.angle)])
        out = np.full(max(F.N, 1), -1, np.int32)
        nm = C.c_int()
        self.ctx.check(lib().coeb_match_keyframe(self.ctx.h, C.byref(camera), C.byref(cf), _p(has), C.byref(kc),
                                                 _p(np.ascontiguousarray(F.mTcw, np.float32)), th, int(ORBdist),
                                                 int(self.mbCheckOrientation), _p(out), C.byref(nm)))
        got = out[:F.N]
        F.mvpMapPoints = np.where(got >= 0, got, F.mvpMapPoints).astype(np.int32)
        return nm.value

    def _search_local_map(self, F, local_map, th=3.0, camera=None):
        if camera is None:
            raise ValueError("SearchByProjection(F, LocalMap, th): camera is required")
        cf = CurFrameC(F.N, C.c_void_p(F.mvKeysUn.ctypes.data), C.c_void_p(F.mDescriptors.ctypes.data),
                       C.c_void_p(F.mvuRight.ctypes.data))
        cobs = np.ascontiguousarray(F.mvpMapPointObs, np.int32)
        lm = local_map.c_struct()
        out = np.full(max(F.N, 1), -1, np.int32)
        nm = C.c_int()
        self.ctx.check(lib().coeb_match_localmap(self.ctx.h, C.byref(camera), C.byref(cf), _p(cobs), C.byref(lm),
                                                 th, self.mfNNratio, _p(out), C.byref(nm)))
        got = out[:F.N]
        hit = got >= 0
        F.mvpMapPoints = np.where(hit, got, F.mvpMapPoints).astype(np.int32)
        if hit.any():
            F.mvpMapPointObs = np.where(hit, local_map.nObs[np.maximum(got, 0)], F.mvpMapPointObs).astype(np.int32)
        return nm.value


class Optimizer:
    """Mirror of ORB_SLAM2::Optimizer for the tracking pose refinement."""

    @staticmethod
    def PoseOptimization(pFrame, camera, ctx):
        F = pFrame
        has = np.ascontiguousarray(F.mvpMapPoints >= 0, np.uint8)
        xw = np.ascontiguousarray(F.mvMapPointPos, np.float32).reshape(F.N, 3) if F.N else np.zeros((1, 3), np.float32)
        fr = PoseFrameC(F.N, C.c_void_p(has.ctypes.data), C.c_void_p(xw.ctypes.data), C.c_void_p(F.mvKeysUn.ctypes.data),
                        C.c_void_p(F.mvuRight.ctypes.data))
        T = np.ascontiguousarray(F.mTcw, np.float32).copy()
        out = np.ascontiguousarray(F.mvbOutlier, np.uint8).copy() if len(F.mvbOutlier) else np.zeros(1, np.uint8)
        nin = C.c_int()
        ctx.check(lib().coeb_pose_optimization(ctx.h, C.byref(camera), C.byref(fr), _p(T), _p(out), C.byref(nin)))
        F.mTcw = T.reshape(4, 4)
        F.mvbOutlier = out[:F.N]
        return nin.value


def make_camera(fx, fy, cx, cy, bf, w, h):
    """Camera + Frame::ComputeImageBounds for an undistorted image (src/Frame.cc:635-641)."""
    return Camera(fx, fy, cx, cy, bf, 0.0, float(w), 0.0, float(h))


# ---- Frame::ProcessMovingObject (src/Frame.cc:311-393) ----
class FlowDebug(C.Structure):
    _fields_ = [("corners_raw", C.c_void_p), ("corners", C.c_void_p), ("ncorners", C.c_void_p),
                ("next_pts", C.c_void_p), ("status", C.c_void_p), ("state", C.c_void_p), ("F", C.c_void_p),
                ("nf", C.c_void_p)]


def _gray(img):
    img = np.ascontiguousarray(img, np.uint8)
    if img.ndim != 2:
        raise ValueError("8UC1 image expected")
    return img, img.shape[1], img.shape[0]


def GoodFeaturesToTrack(ctx, img, max_corners=1000, quality=0.01, min_distance=8.0, k=0.04):
    """cv::goodFeaturesToTrack(img, corners, maxCorners, quality, minDistance, Mat(), 3, true, k)
    as Frame.cc:333 calls it: (n, 2) float32."""
    img, w, h = _gray(img)
    out = np.zeros((max_corners, 2), np.float32)
    n = C.c_int(0)
    ctx.check(lib().coeb_good_features(ctx.h, _p(img), w, h, w, max_corners, quality, min_distance, k, _p(out),
                                       max_corners, C.byref(n)))
    return out[:n.value].copy()


def CornerSubPix(ctx, img, xy, win=10, max_iter=20, eps=0.03):
    """cv::cornerSubPix(img, xy, Size(win, win), Size(-1,-1), TermCriteria(ITER|EPS, max_iter, eps))
    (Frame.cc:334); returns the refined copy."""
    img, w, h = _gray(img)
    xy = np.ascontiguousarray(xy, np.float32).copy()
    ctx.check(lib().coeb_corner_subpix(ctx.h, _p(img), w, h, w, _p(xy), len(xy), win, max_iter, eps))
    return xy


def CalcOpticalFlowPyrLK(ctx, prev, nxt, xy, win=22, max_level=5, max_count=20, eps=0.01):
    """cv::calcOpticalFlowPyrLK(prev, next, xy, next_xy, status, err, Size(win, win), max_level,
    TermCriteria(ITER|EPS, max_count, eps)) (Frame.cc:335): (next_xy, status)."""
    prev, w, h = _gray(prev)
    nxt = np.ascontiguousarray(nxt, np.uint8)
    xy = np.ascontiguousarray(xy, np.float32)
    out = np.zeros_like(xy)
    st = np.zeros(len(xy), np.uint8)
    ctx.check(lib().coeb_optical_flow_pyr_lk(ctx.h, _p(prev), _p(nxt), w, h, w, _p(xy), len(xy), win, max_level,
                                             max_count, eps, _p(out), _p(st)))
    return out, st


def MovingTail(ctx, prev, cur, pxy, nxy, state):
    """SAD check + cv::findFundamentalMat(FM_RANSAC, 0.1, 0.99) + epipolar test (Frame.cc:337-384):
    (T_M or None when F is empty, state after the SAD check, F or None, |F_prepoint|)."""
    prev, w, h = _gray(prev)
    cur = np.ascontiguousarray(cur, np.uint8)
    pxy = np.ascontiguousarray(pxy, np.float32)
    nxy = np.ascontiguousarray(nxy, np.float32)
    st = np.ascontiguousarray(state, np.uint8).copy()
    tm = np.zeros((max(len(pxy), 1), 2), np.float32)
    F = np.zeros(9, np.float64)
    nt, nf = C.c_int(0), C.c_int(0)
    ctx.check(lib().coeb_moving_tail(ctx.h, _p(prev), _p(cur), w, h, w, _p(pxy), _p(nxy), _p(st), len(pxy), _p(tm),
                                     len(tm), C.byref(nt), _p(F), C.byref(nf)))
    if nt.value < 0:
        return None, st, None, nf.value
    return tm[:nt.value].copy(), st, F.reshape(3, 3), nf.value


def ProcessMovingObject(ctx, prev, cur, debug=False):
    """Frame::ProcessMovingObject(imgray, box) with imGrayPre = prev (Frame.cc:311-393): T_M as
    (m, 2) float32, or None when findFundamentalMat returns an empty Mat.  debug=True also
    returns the stage outputs (dict)."""
    prev, w, h = _gray(prev)
    cur = np.ascontiguousarray(cur, np.uint8)
    tm = np.zeros((1024, 2), np.float32)
    nt = C.c_int(0)
    dbg, arrays = None, None
    if debug:
        arrays = dict(corners_raw=np.zeros((1000, 2), np.float32), corners=np.zeros((1000, 2), np.float32),
                      ncorners=np.zeros(1, np.int32), next_pts=np.zeros((1000, 2), np.float32),
                      status=np.zeros(1000, np.uint8), state=np.zeros(1000, np.uint8), F=np.zeros(9, np.float64),
                      nf=np.zeros(1, np.int32))
        dbg = FlowDebug(**{k: _p(v) for k, v in arrays.items()})
    ctx.check(lib().coeb_moving_object_points(ctx.h, _p(prev), _p(cur), w, h, w, _p(tm), len(tm), C.byref(nt),
                                              C.byref(dbg) if dbg is not None else None))
    res = None if nt.value < 0 else tm[:nt.value].copy()
    if not debug:
        return res
    n = int(arrays["ncorners"][0])
    arrays["ncorners"] = n
    arrays["nf"] = int(arrays["nf"][0])
    for k in ("corners_raw", "corners", "next_pts", "status", "state"):
        arrays[k] = arrays[k][:n]
    arrays["F"] = arrays["F"].reshape(3, 3)
    return res, arrays
