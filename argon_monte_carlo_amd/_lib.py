"""Loader of libargonmc.so (the HIP/gfx950 C-ABI library, include/argonmc.h).

There is deliberately no fallback: if the library is missing or no MI355X is usable, the product path raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

from ._abi import (AMC_ABI_VERSION, AmcCorrGrid, AmcFieldGrid, AmcFluxGrid, AmcIcConfig, AmcMfpGrid, AmcParams, AmcPathRecord, AmcStepStats, AmcSurfaceGrid,
                   AmcPairGrid, AmcTempRng, AmcTransitGrid, AmcVdfGrid, AmcWallLaw)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libargonmc.so")
_LIB = None

_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_ctx = C.c_void_p

# every symbol include/argonmc.h declares: (restype, argtypes)
SIGNATURES = {
    "amc_abi_version": (C.c_int, []),
    "amc_create": (C.c_int, [C.POINTER(_ctx), C.POINTER(AmcParams)]),
    "amc_destroy": (None, [_ctx]),
    "amc_last_error": (C.c_char_p, [_ctx]),
    "amc_set_stream": (C.c_int, [_ctx, C.c_void_p]),
    "amc_use_null_stream": (C.c_int, [_ctx]),
    "amc_synchronize": (C.c_int, [_ctx]),
    "amc_upload": (C.c_int, [_ctx] + [_dp] * 10 + [_u8p]),
    "amc_download": (C.c_int, [_ctx] + [_dp] * 10 + [_u8p]),
    "amc_download_prior": (C.c_int, [_ctx, _dp, _dp, _dp]),
    "amc_timestep": (C.c_int, [_ctx, C.c_double, C.POINTER(AmcStepStats)]),
    "amc_run": (C.c_int, [_ctx, C.c_double, C.c_int64, C.POINTER(AmcStepStats)]),
    "amc_stage_drift": (C.c_int, [_ctx, C.c_double]),
    "amc_stage_walls": (C.c_int, [_ctx, C.POINTER(AmcStepStats)]),
    "amc_stage_bounds": (C.c_int, [_ctx, _i64p]),
    "amc_stage_sweep": (C.c_int, [_ctx, C.POINTER(AmcStepStats)]),
    "amc_pairwise_cell": (C.c_int, [_ctx, C.c_int64] + [_dp] * 4 + [_u8p] + [_dp] * 6 + [_dp, C.c_size_t,
                                                                                       C.POINTER(C.c_size_t), _i64p]),
    "amc_temp_begin": (C.c_int, [_ctx, C.c_double]),
    "amc_temp_end": (C.c_int, [_ctx, C.POINTER(AmcStepStats)]),
    "amc_temp_cases_device": (C.c_int, [_ctx, C.POINTER(AmcTempRng)]),
    "amc_temp_device_results": (C.c_int, [_ctx, C.c_int, _i32p, _dp, _dp, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "amc_temp_device_sums": (C.c_int, [_ctx, _dp, C.POINTER(C.c_int32)]),
    "amc_temp_device_draws": (C.c_int, [_ctx, C.c_int, _i32p, _dp, _dp, _dp, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "amc_temp_run_device": (C.c_int, [_ctx, C.c_double, C.c_int64, C.POINTER(AmcTempRng), C.POINTER(AmcStepStats)]),
    "amc_temp_series_read": (C.c_int, [_ctx, C.c_int64, C.c_int64, _dp, _u8p, _i64p]),
    "amc_set_step": (C.c_int, [_ctx, C.c_int64]),
    "amc_host_directions": (C.c_int, [C.POINTER(C.c_uint32), _i32p, C.POINTER(C.c_uint32), _i32p, _dp, _u8p, C.c_int64, C.c_double,
                                      C.c_double, C.c_int, C.c_void_p, _dp]),
    "amc_wall_hits": (C.c_int, [_ctx, C.c_int, _i32p, _dp, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "amc_wall_apply": (C.c_int, [_ctx, C.c_int, _dp, _dp, C.c_size_t, _dp, _dp]),
    "amc_wall_park": (C.c_int, [_ctx, C.c_int, _dp, C.c_size_t]),
    "amc_wall_finish": (C.c_int, [_ctx, C.c_int, _dp, C.c_size_t, _dp, _dp]),
    "amc_wall_hits_again": (C.c_int, [_ctx]),
    "amc_drain_paths": (C.c_int, [_ctx, C.POINTER(AmcPathRecord), C.c_size_t, C.POINTER(C.c_size_t)]),
    "amc_paths_pending": (C.c_int, [_ctx, C.POINTER(C.c_size_t)]),
    "amc_histograms": (C.c_int, [_ctx, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "amc_reset_outputs": (C.c_int, [_ctx]),
    "amc_init_synthetic": (C.c_int, [_ctx, C.POINTER(AmcIcConfig)]),
    "amc_set_shard": (C.c_int, [_ctx, C.c_int64, C.c_int64]),
    "amc_mg_local": (C.c_int, [_ctx, C.c_double]),
    "amc_mg_exchange_view": (C.c_int, [_ctx, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "amc_mg_pack": (C.c_int, [_ctx, C.c_int]),
    "amc_mg_sweep": (C.c_int, [_ctx, C.c_int, C.c_int]),
    "amc_mg_candidates_view": (C.c_int, [_ctx, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "amc_mg_detect": (C.c_int, [_ctx, C.c_int, C.c_int]),
    "amc_mg_resolve": (C.c_int, [_ctx, C.c_int]),
    "amc_mg_bounds": (C.c_int, [_ctx]),
    "amc_mg_finish": (C.c_int, [_ctx, C.POINTER(AmcStepStats)]),
    "amc_profile": (C.c_int, [_ctx, C.c_int]),
    "amc_kernel_times": (C.c_int, [_ctx, _dp, _i64p]),
    "amc_kernel_name": (C.c_char_p, [C.c_int]),
    "amc_overlap_stats": (C.c_int, [_ctx, _i64p]),
    "amc_lists_stats": (C.c_int, [_ctx, _i64p]),
    "amc_owned_count": (C.c_int, [_ctx, _i64p]),
    "amc_fields_config": (C.c_int, [_ctx, C.POINTER(AmcFieldGrid)]),
    "amc_fields_sample": (C.c_int, [_ctx]),
    "amc_fields_read": (C.c_int, [_ctx, _i64p, _i64p, _i64p]),
    "amc_fields_load": (C.c_int, [_ctx, _i64p, C.c_int64, C.c_int64]),
    "amc_fields_reset": (C.c_int, [_ctx]),
    "amc_surface_config": (C.c_int, [_ctx, C.POINTER(AmcSurfaceGrid)]),
    "amc_surface_read": (C.c_int, [_ctx, _i64p, _i64p, _i64p]),
    "amc_surface_load": (C.c_int, [_ctx, _i64p, _i64p, C.c_int64]),
    "amc_surface_reset": (C.c_int, [_ctx]),
    "amc_temp_device_contacts": (C.c_int, [_ctx, C.c_int, _i32p, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "amc_wall_contacts": (C.c_int, [_ctx, C.c_int, _dp, C.c_size_t]),
}

# ... and every symbol include/argonmc_corr.h declares (the sampled correlations; argonmc.h includes it)
CORR_SIGNATURES = {
    "amc_corr_config": (C.c_int, [_ctx, C.POINTER(AmcCorrGrid)]),
    "amc_corr_sample": (C.c_int, [_ctx]),
    "amc_corr_read": (C.c_int, [_ctx, _i64p, _i64p, _i64p, _i64p, _i64p]),
    "amc_corr_origin": (C.c_int, [_ctx] + [_dp] * 6),
    "amc_corr_load": (C.c_int, [_ctx, _i64p, C.c_int64, C.c_int64, C.c_int64, C.c_int64] + [_dp] * 6),
    "amc_corr_reset": (C.c_int, [_ctx]),
}

# ... and every symbol include/argonmc_flux.h declares (the sampled fluxes; argonmc.h includes it)
FLUX_SIGNATURES = {
    "amc_flux_config": (C.c_int, [_ctx, C.POINTER(AmcFluxGrid)]),
    "amc_flux_sample": (C.c_int, [_ctx]),
    "amc_flux_read": (C.c_int, [_ctx, _i64p, _i64p, _i64p]),
    "amc_flux_load": (C.c_int, [_ctx, _i64p, C.c_int64, C.c_int64]),
    "amc_flux_reset": (C.c_int, [_ctx]),
}

# ... and every symbol include/argonmc_mfp.h declares (the sampled free paths; argonmc.h includes it)
MFP_SIGNATURES = {
    "amc_mfp_config": (C.c_int, [_ctx, C.POINTER(AmcMfpGrid)]),
    "amc_mfp_read": (C.c_int, [_ctx, _i64p, _i64p, _i64p, _i64p, _i64p]),
    "amc_mfp_load": (C.c_int, [_ctx, _i64p, _i64p, C.c_int64, C.c_int64, C.c_int64]),
    "amc_mfp_reset": (C.c_int, [_ctx]),
}

# ... and every symbol include/argonmc_vdf.h declares (the sampled velocity distributions; argonmc.h includes it)
VDF_SIGNATURES = {
    "amc_vdf_config": (C.c_int, [_ctx, C.POINTER(AmcVdfGrid)]),
    "amc_vdf_sample": (C.c_int, [_ctx]),
    "amc_vdf_read": (C.c_int, [_ctx, _i64p, _i64p, _i64p]),
    "amc_vdf_load": (C.c_int, [_ctx, _i64p, C.c_int64, C.c_int64]),
    "amc_vdf_reset": (C.c_int, [_ctx]),
}

# ... and every symbol include/argonmc_transit.h declares (the sampled transits; argonmc.h includes it)
_u32p = C.POINTER(C.c_uint32)
TRANSIT_SIGNATURES = {
    "amc_transit_config": (C.c_int, [_ctx, C.POINTER(AmcTransitGrid)]),
    "amc_transit_sample": (C.c_int, [_ctx]),
    "amc_transit_read": (C.c_int, [_ctx, _i64p, _i64p]),
    "amc_transit_state": (C.c_int, [_ctx, _u32p, _u32p]),
    "amc_transit_load": (C.c_int, [_ctx, _i64p, C.c_int64, _u32p, _u32p]),
    "amc_transit_reset": (C.c_int, [_ctx]),
}

# ... and every symbol include/argonmc_pair.h declares (the sampled pair distribution; argonmc.h includes it)
PAIR_SIGNATURES = {
    "amc_pair_config": (C.c_int, [_ctx, C.POINTER(AmcPairGrid)]),
    "amc_pair_sample": (C.c_int, [_ctx]),
    "amc_pair_read": (C.c_int, [_ctx, _i64p, _i64p, _i64p, _i64p]),
    "amc_pair_load": (C.c_int, [_ctx, _i64p, C.c_int64, C.c_int64, C.c_int64]),
    "amc_pair_reset": (C.c_int, [_ctx]),
}

# ... and every symbol include/argonmc_shard.h declares (the device-RNG energised pore over shards; argonmc.h includes it)
SHARD_SIGNATURES = {
    "amc_mg_hits_view": (C.c_int, [_ctx, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "amc_mg_hits_pack": (C.c_int, [_ctx, C.c_int]),
    "amc_mg_hits_sums": (C.c_int, [_ctx, C.c_int, C.c_int64]),
    "amc_temp_shard_run_begin": (C.c_int, [_ctx, C.c_int64]),
    "amc_temp_shard_run_end": (C.c_int, [_ctx, C.c_int64, C.POINTER(AmcStepStats)]),
}

# ... and every symbol include/argonmc-ic.h declares (the overlap removal of a synthetic start; argonmc.h includes it)
IC_SIGNATURES = {
    "amc_init_separate": (C.c_int, [_ctx, C.POINTER(AmcIcConfig), C.c_double, C.c_int32, C.c_int32, _i64p]),
}

# ... and every symbol include/argonmc-walllaw.h declares (the device-RNG steps' wall law; argonmc.h includes it).  A table beside
# all_signatures(), whose size tests/test_ic_separate_host.py fixes: load() types both (typed_signatures)
WALL_LAW_SIGNATURES = {
    "amc_temp_wall_law": (C.c_int, [_ctx, C.POINTER(AmcWallLaw)]),
    "amc_temp_wall_law_get": (C.c_int, [_ctx, C.POINTER(AmcWallLaw)]),
}


def all_signatures():
    """every entry point of the library: the tables above, one per header, in one dict"""
    return {**SIGNATURES, **SHARD_SIGNATURES, **CORR_SIGNATURES, **FLUX_SIGNATURES, **MFP_SIGNATURES, **VDF_SIGNATURES, **TRANSIT_SIGNATURES,
            **PAIR_SIGNATURES, **IC_SIGNATURES}


def typed_signatures():
    """what load() types: all_signatures() and the wall law's entry points"""
    return {**all_signatures(), **WALL_LAW_SIGNATURES}


class ArgonMCError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libargonmc error {code}: {msg}")
        self.code = code


def build(verbose=False):
    """Compile libargonmc.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j4"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    if verbose or r.returncode != 0:
        print(r.stdout.decode(errors="replace")[-4000:])
    if r.returncode != 0:
        raise RuntimeError("building libargonmc.so failed")
    with open(STAMP_PATH, "w") as fh:
        fh.write(source_digest() + "\n")
    return LIB_PATH


STAMP_PATH = LIB_PATH + ".sources"


def _source_files():
    src_dir = os.path.join(_HERE, "csrc")
    files = [os.path.join(src_dir, f) for f in sorted(os.listdir(src_dir)) if f.endswith((".hip", ".h")) or f == "Makefile"]
    files.append(os.path.join(os.path.dirname(_HERE), "include", "argonmc.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "argonmc_shard.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "argonmc_corr.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "argonmc_flux.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "argonmc_mfp.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "argonmc_vdf.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "argonmc_transit.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "argonmc_pair.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "argonmc-ic.h"))
    files.append(os.path.join(os.path.dirname(_HERE), "include", "argonmc-walllaw.h"))
    return files


def source_digest():
    """sha256 over the library's sources (csrc/*.hip, csrc/*.h, the Makefile, include/argonmc.h, argonmc_shard.h, argonmc_corr.h,
    argonmc_flux.h, argonmc_mfp.h, argonmc_vdf.h, argonmc_transit.h, argonmc_pair.h, argonmc-ic.h and argonmc-walllaw.h)."""
    import hashlib
    h = hashlib.sha256()
    for f in _source_files():
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def stale_sources():
    """Non-empty when the built libargonmc.so does not belong to the sources in the tree.  The .so is not under version
    control (it travels with the working tree, and file times do not survive every copy): build() leaves the digest of
    the sources it compiled next to it, and a library without a matching digest is refused — it would silently run old
    kernels."""
    if not os.path.exists(LIB_PATH):
        return []
    try:
        with open(STAMP_PATH) as fh:
            built = fh.read().strip()
    except OSError:
        return ["(no source digest next to the library)"]
    return [] if built == source_digest() else ["(sources changed since the library was built)"]


def load():
    """dlopen libargonmc.so and type every entry point.  Raises if the library is absent — there is no CPU path."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ArgonMCError(-2, f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(no CPU fallback exists)")
    stale = stale_sources()
    if stale:
        raise ArgonMCError(-3, f"{LIB_PATH} does not match the sources {stale[0]}: rebuild it "
                               "(`python -c 'import __graft_entry__ as g; g.build()'`)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in typed_signatures().items():
        fn = getattr(lib, name)          # AttributeError = missing export
        fn.restype = res
        fn.argtypes = args
    if lib.amc_abi_version() != AMC_ABI_VERSION:
        raise ArgonMCError(-1, "ABI version mismatch between _abi.py and libargonmc.so")
    _LIB = lib
    return lib
