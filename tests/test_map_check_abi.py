"""CPU: the batched map check's entry points (include/csm_map_check.h, and
csm_loop_closure_map_check) exist, their parameter struct has the header's
layout, and what can be refused without a device is refused: null arguments
(a call with check_point_num == 1 and a two-point scan among them; that rule
itself needs a map and is tested on the GPU). No GPU."""
import ctypes as C

import numpy as np

from roborts_csm import _abi

NEW = ("csm_gridmap_feedback_penalty_batch", "csm_gridmap_feedback_penalty_store",
       "csm_gridmap_map_check_launches", "csm_gridmap_feedback_penalty_store_kernel_ms",
       "csm_loop_closure_map_check")
_dp = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)


def test_symbols_exist_and_are_bound():
    raw = C.CDLL(_abi.LIB_PATH)
    lib = _abi.load_library()
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _abi.EXPORTED, name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.csm_abi_version() == 1


def test_param_struct_layout():
    P = _abi.CsmMapCheckParam
    assert C.sizeof(P) == 4 * 4 + 2 * 8
    assert [f[0] for f in P._fields_] == ["check_point_num", "use_blur", "use_logistic", "reserved",
                                          "bound_tolerance", "penalty_gain"]
    assert (P.check_point_num.offset, P.use_blur.offset, P.use_logistic.offset, P.reserved.offset,
            P.bound_tolerance.offset, P.penalty_gain.offset) == (0, 4, 8, 12, 16, 24)


def _args(n_points=2, cpn=50):
    pts = np.zeros((n_points, 2))
    off = np.array([0, n_points], dtype=np.int64)
    pose = np.zeros(3)
    prm = _abi.CsmMapCheckParam(cpn, 0, 1, 0, 2.5, 0.015)
    coeff = np.full(1, -7.0)
    counts = np.full(1, -7, dtype=np.int32)
    return pts, off, pose, prm, coeff, counts


def test_null_arguments_are_rejected():
    lib = _abi.load_library()
    pts, off, pose, prm, coeff, counts = _args()
    E = _abi.CSM_ERR_INVALID_ARG
    assert lib.csm_gridmap_feedback_penalty_batch(None, 1, pts.ctypes.data_as(_dp), off.ctypes.data_as(_i64p), 1, None,
                                                  pose.ctypes.data_as(_dp), C.byref(prm), coeff.ctypes.data_as(_dp),
                                                  counts.ctypes.data_as(_i32p)) == E
    ids = np.zeros(1, dtype=np.int32)
    assert lib.csm_gridmap_feedback_penalty_store(None, None, 1, ids.ctypes.data_as(_i32p), pose.ctypes.data_as(_dp),
                                                  C.byref(prm), coeff.ctypes.data_as(_dp), None) == E
    n, ms = C.c_int64(-1), C.c_double(-1.0)
    assert lib.csm_gridmap_map_check_launches(None, C.byref(n)) == E
    assert lib.csm_gridmap_feedback_penalty_store_kernel_ms(None, None, 1, ids.ctypes.data_as(_i32p),
                                                            pose.ctypes.data_as(_dp), C.byref(prm), 1,
                                                            C.byref(ms)) == E
    res = (_abi.CsmLoopClosureResult * 1)()
    assert lib.csm_loop_closure_map_check(None, None, 0, C.byref(prm), res, 1, coeff.ctypes.data_as(_dp)) == E
    assert coeff[0] == -7.0 and counts[0] == -7 and n.value == -1  # nothing was written


def test_one_check_point_with_two_points_is_rejected():
    """check_point_num == 1 with a scan of two points: the reference divides
    by zero (occu_grid_map.h:368). No map can be made without a device, so
    here the call names no map and the null argument alone already refuses
    it: this only shows that such a call is refused and writes nothing. The
    rule itself is tested on a real map in tests/test_gpu_map_check_batch.py
    (test_guard_and_rejected_arguments)."""
    lib = _abi.load_library()
    pts, off, pose, prm, coeff, counts = _args(n_points=2, cpn=1)
    assert lib.csm_gridmap_feedback_penalty_batch(None, 1, pts.ctypes.data_as(_dp), off.ctypes.data_as(_i64p), 1, None,
                                                  pose.ctypes.data_as(_dp), C.byref(prm), coeff.ctypes.data_as(_dp),
                                                  counts.ctypes.data_as(_i32p)) == _abi.CSM_ERR_INVALID_ARG
    assert coeff[0] == -7.0 and counts[0] == -7
