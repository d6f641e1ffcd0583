"""CPU: the NIS gate's C-ABI surface and EkfSlam.set_nis_gate's arguments, with the library's calls stubbed (no device)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_declare_the_gate():
    text = open(os.path.join(ROOT, "include", "ekfslam_hip.h")).read()
    want = {
        "ekf_set_nis_gate": ["ekf_handle *h", "double threshold"],
        "ekf_download_gate_counts": ["ekf_handle *h", "int b0", "int count", "long long *rejected"],
        "ekf_download_innovation_rejections": ["ekf_handle *h", "long long first", "int count", "int *rejected"],
    }
    from slam_duckietown_amd import ekf_bindings as eb
    types = {
        "ekf_set_nis_gate": [C.c_void_p, C.c_double],
        "ekf_download_gate_counts": [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_longlong)],
        "ekf_download_innovation_rejections": [C.c_void_p, C.c_longlong, C.c_int, eb._ip],
    }
    for name, params in want.items():
        decl = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert decl, f"{name} is not declared in include/ekfslam_hip.h"
        assert [p.strip() for p in decl.group(1).split(",")] == params
        res, args = eb.ABI[name]
        assert res is C.c_int and args == types[name]


class _Lib:
    """Records what the binding hands to the library."""

    def __init__(self):
        self.calls = []

    def ekf_set_nis_gate(self, h, threshold):
        self.calls.append(threshold)
        return 0

    def ekf_last_error(self, h):
        return b""


def _filter():
    from slam_duckietown_amd.ekf_bindings import EkfSlam
    f = object.__new__(EkfSlam)                  # (no device: only the stubbed library is reached)
    f._lib = _Lib()
    f._h = C.c_void_p()
    return f


@pytest.mark.parametrize("p", [0.95, 0.99, 0.999])
def test_confidence_passes_the_chi2_quantile(p):
    from scipy.stats import chi2
    f = _filter()
    f.set_nis_gate(confidence=p)
    (g,) = f._lib.calls
    assert g == pytest.approx(chi2.ppf(p, 2), rel=1e-9)
    # the gate nis_consistency counts "above" against is the same number
    from slam_duckietown_amd.evaluation import nis_consistency
    from slam_duckietown_amd.ekf_bindings import Innovations
    nis = np.array([[[0.5 * g, 2.0 * g]]])
    innov = Innovations(np.arange(1), np.array([[2]]), np.zeros((1, 1, 2), dtype=np.int32), np.zeros((1, 1, 2, 2)),
                        np.broadcast_to(np.eye(2), (1, 1, 2, 2, 2)).copy(), nis)
    r = nis_consistency(innov, confidence=p)
    assert r.gate == pytest.approx(g, rel=1e-9) and r.above_gate == pytest.approx(0.5)


def test_thresholds_and_off():
    f = _filter()
    f.set_nis_gate(9.5)
    f.set_nis_gate(None)
    f.set_nis_gate(threshold=math.inf)
    f.set_nis_gate()
    assert f._lib.calls[0] == 9.5 and all(math.isinf(g) and g > 0 for g in f._lib.calls[1:])


@pytest.mark.parametrize("kw", [dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")),
                                dict(threshold=-math.inf), dict(confidence=0.0), dict(confidence=1.0),
                                dict(confidence=1.5), dict(confidence=float("nan")), dict(threshold=5.0, confidence=0.9)])
def test_bad_arguments_are_refused_without_a_device(kw):
    f = _filter()
    with pytest.raises(ValueError):
        f.set_nis_gate(**kw)
    assert f._lib.calls == []


def test_innovations_keeps_its_six_positional_fields():
    from slam_duckietown_amd.ekf_bindings import Innovations
    z = np.zeros((1, 1, 1))
    i = Innovations(np.arange(1), np.ones((1, 1), dtype=np.int32), z.astype(np.int32), np.zeros((1, 1, 1, 2)),
                    np.zeros((1, 1, 1, 2, 2)), z)
    assert i.rejected is None and Innovations._fields[-1] == "rejected"
