"""cu-sdr-collection_amd — MI355X-native acquisition + tracking hot path for the
CU-SDR-Collection GNSS software receivers.

Layout: csrc/ (HIP kernels + the C-ABI of include/gnsscorr.h), _lib.py (ctypes binding),
engine.py (context wrapper), receiver.py (acquisition / preRun / tracking with the reference's
names and struct fields), codes.py (code generators), settings.py (initSettings mirror),
synth.py (synthetic IF records).  Nothing here imports `oracle/`; there is no CPU fallback.
"""
from . import _lib, acq_family, acq_shift, codes, nav_sync, settings, signals, synth  # noqa: F401
from ._lib import GnssCorrError  # noqa: F401
from .engine import Engine, device_count  # noqa: F401
from .receiver import CNoVSM, acquisition, bit_edge_search, cancel_tracked, correlation_function, excise_interference, excise_swept, downconvert_band, resample_record, null_steer, array_covariance_matrix, power_inversion_weights, mvdr_weights, delay_doppler_map, integrated_delay_doppler_map, secondary_code_search, preRun, probeData, tracking, tracking_file, tracking_multi  # noqa: F401
from .settings import initSettings  # noqa: F401

__all__ = ["Engine", "device_count", "GnssCorrError", "probeData", "acquisition", "preRun", "tracking", "tracking_file", "tracking_multi", "correlation_function", "delay_doppler_map", "integrated_delay_doppler_map", "bit_edge_search", "secondary_code_search", "cancel_tracked", "excise_interference", "excise_swept", "downconvert_band", "resample_record", "null_steer", "array_covariance_matrix", "power_inversion_weights", "mvdr_weights", "CNoVSM", "initSettings",
           "codes", "settings", "synth"]
