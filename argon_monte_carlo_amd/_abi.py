"""ctypes mirror of include/argonmc.h (structs only; no library is loaded here)."""
import ctypes as C

AMC_ABI_VERSION = 2

AMC_OK = 0
AMC_ERR_INVALID = -1
AMC_ERR_NO_DEVICE = -2
AMC_ERR_HIP = -3
AMC_ERR_CAPACITY = -4
AMC_ERR_FP = -5
AMC_ERR_STATE = -6

AMC_GEOM_CELL = 0
AMC_GEOM_CUBE = 1
AMC_GEOM_PORE = 2
AMC_GEOM_PORE_ENERGISED = 3

_D = C.c_double


class AmcParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("geometry", C.c_int32), ("n", C.c_int64),
        ("collision_range", _D), ("argon_mass", _D), ("argon_radius", _D),
        ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("reserved0", C.c_int32),
        ("dx", _D), ("dy", _D), ("dz", _D),
        ("overlap_x", _D), ("overlap_y", _D), ("overlap_z", _D),
        ("cube_x", _D), ("cube_y", _D), ("cube_z", _D),
        ("R_oa", _D), ("R_oa_c", _D), ("R_p", _D), ("R_p_c", _D), ("R_g", _D), ("R_g_c", _D),
        ("H", _D), ("h_oa", _D), ("z_cold", _D), ("z_gap_bottom", _D), ("z_gap_top", _D),
        ("oob_z_lo_fix", _D), ("oob_z_hi_fix", _D),
        ("R_oa_sq", _D), ("R_g_sq", _D), ("R_p_sq", _D),
        ("z_oob_hot_top", _D), ("z_oob_gap_top", _D),
        ("t_z3_cold", _D), ("t_z3_hot", _D), ("t_zgap_lo", _D), ("t_zgap_hi", _D),
        ("R_g_c_sq", _D), ("R_p_c_sq", _D),
        ("E_cold", _D), ("E_hot", _D), ("alpha_coated", _D), ("alpha_gap", _D), ("cos85", _D),
        ("hist_bins", C.c_int32), ("reserved1", C.c_int32), ("hist_lo", _D), ("hist_hi", _D),
        ("fine_cell", _D), ("device", C.c_int32), ("detect_mode", C.c_int32),
        ("max_candidates", C.c_int64), ("max_paths", C.c_int64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    @classmethod
    def from_dict(cls, d):
        p = cls()
        for k, _ in cls._fields_:
            if k in d:
                v = d[k]
                setattr(p, k, v.item() if hasattr(v, "item") else v)
        p.struct_size = C.sizeof(cls)
        return p


class AmcStepStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in (
        "n_pp", "n_wall", "n_oob_walls", "n_oob_pp", "n_paths", "n_candidates", "n_clusters", "n_rounds",
        "n_fp_errors", "flags")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class AmcPathRecord(C.Structure):
    _fields_ = [("step", C.c_int32), ("phase", C.c_int32), ("cell", C.c_int64), ("i", C.c_int32), ("j", C.c_int32),
                ("which", C.c_int32), ("reserved", C.c_int32), ("total", _D), ("px", _D), ("py", _D), ("pz", _D)]


class AmcIcConfig(C.Structure):
    """amc_ic_config (include/argonmc.h): synthetic initial conditions generated on the device."""
    _fields_ = [("struct_size", C.c_int32), ("n_regions", C.c_int32), ("seed", C.c_uint64), ("a_shape", C.c_double),
                ("first", C.c_int64 * 9), ("radius", C.c_double * 8), ("z_lo", C.c_double * 8), ("z_hi", C.c_double * 8)]


class AmcTempRng(C.Structure):
    """amc_temp_rng (include/argonmc.h): configuration of the opt-in device-side energised-wall sampling."""
    _fields_ = [("struct_size", C.c_int32), ("n_gl", C.c_int32), ("seed", C.c_uint64),
                ("t_cold", C.c_double), ("t_hot", C.c_double), ("gap_height", C.c_double), ("gap_bottom_height", C.c_double),
                ("t_debye_alumina", C.c_double), ("n_alumina", C.c_double), ("boltzman", C.c_double),
                ("gl_x", C.c_double * 32), ("gl_w", C.c_double * 32)]


AMC_WALL_LAW_REFERENCE = 0
AMC_WALL_LAW_MAXWELL = 1


class AmcWallLaw(C.Structure):
    """amc_wall_law (include/argonmc-walllaw.h): the wall law of the device-RNG energised steps."""
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("alpha_coated", C.c_double), ("alpha_gap", C.c_double),
                ("reserved", C.c_double * 4)]


AMC_FIELDS_CARTESIAN = 0
AMC_FIELDS_AXISYMMETRIC = 1
AMC_FIELDS_MAX_BINS = 2048


class AmcFieldGrid(C.Structure):
    """amc_field_grid (include/argonmc.h): the bins of the sampled fields and the sampling cadence."""
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("n1", C.c_int32), ("n2", C.c_int32), ("n3", C.c_int32),
                ("reserved", C.c_int32), ("every", C.c_int64), ("step_offset", C.c_int64),
                ("lo", C.c_double * 3), ("hi", C.c_double * 3)]


AMC_CORR_MAX_GROUPS = 256
AMC_CORR_MAX_CELLS = 65536


class AmcCorrGrid(C.Structure):
    """amc_corr_grid (include/argonmc.h): the groups, the lags and the cadence of the sampled correlations."""
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("n1", C.c_int32), ("n2", C.c_int32), ("n3", C.c_int32),
                ("n_lags", C.c_int32), ("every", C.c_int64), ("step_offset", C.c_int64),
                ("lo", C.c_double * 3), ("hi", C.c_double * 3), ("reserved", C.c_int64 * 2)]


AMC_FLUX_MAX_BINS = 1024


class AmcFluxGrid(C.Structure):
    """amc_flux_grid (include/argonmc_flux.h): the bins of the sampled fluxes and the sampling cadence; the fields of amc_field_grid."""
    _fields_ = list(AmcFieldGrid._fields_)


AMC_MFP_MAX_COLUMNS = 6144
AMC_MFP_MAX_HIST_BINS = 64


class AmcMfpGrid(C.Structure):
    """amc_mfp_grid (include/argonmc_mfp.h): the bins of the sampled free paths, their histogram and what becomes of the records."""
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("n1", C.c_int32), ("n2", C.c_int32), ("n3", C.c_int32),
                ("hist_bins", C.c_int32), ("keep_records", C.c_int32), ("reserved", C.c_int32),
                ("lo", C.c_double * 3), ("hi", C.c_double * 3), ("hist_hi", C.c_double)]


AMC_VDF_MAX_HIST_BINS = 256
AMC_VDF_MAX_COLUMNS = 24576


class AmcVdfGrid(C.Structure):
    """amc_vdf_grid (include/argonmc_vdf.h): the regions of the sampled velocity distributions, their histograms and the cadence."""
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("n1", C.c_int32), ("n2", C.c_int32), ("n3", C.c_int32),
                ("hist_bins", C.c_int32), ("every", C.c_int64), ("step_offset", C.c_int64),
                ("lo", C.c_double * 3), ("hi", C.c_double * 3), ("v_max", C.c_double), ("reserved", C.c_int64 * 2)]


AMC_TRANSIT_MAX_ZONES = 8
AMC_TRANSIT_HIST = 40
AMC_TRANSIT_CLASS_COLUMNS = 43
AMC_TRANSIT_COLUMNS = 263
AMC_TRANSIT_MAX_SAMPLES = 2 ** 32 - 1


class AmcTransitGrid(C.Structure):
    """amc_transit_grid (include/argonmc_transit.h): the zones of the sampled transits and the cadence."""
    _fields_ = [("struct_size", C.c_int32), ("n_zones", C.c_int32), ("every", C.c_int64), ("step_offset", C.c_int64),
                ("axis", C.c_int32 * AMC_TRANSIT_MAX_ZONES), ("lo", C.c_double * AMC_TRANSIT_MAX_ZONES),
                ("hi", C.c_double * AMC_TRANSIT_MAX_ZONES), ("reserved", C.c_int64 * 2)]


AMC_PAIR_MAX_HIST_BINS = 256
AMC_PAIR_MAX_COLUMNS = 6144
AMC_PAIR_MAX_CELLS_AXIS = 128


class AmcPairGrid(C.Structure):
    """amc_pair_grid (include/argonmc_pair.h): the regions of the sampled pair distribution, its histogram and the cadence."""
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("n1", C.c_int32), ("n2", C.c_int32), ("n3", C.c_int32),
                ("hist_bins", C.c_int32), ("every", C.c_int64), ("step_offset", C.c_int64),
                ("lo", C.c_double * 3), ("hi", C.c_double * 3), ("r_max", C.c_double), ("reserved", C.c_int64 * 2)]


AMC_SURFACE_CASES = 7
AMC_SURFACE_MAX_BINS = 256


class AmcSurfaceGrid(C.Structure):
    """amc_surface_grid (include/argonmc.h): the wall bins of the sampled surfaces, [case - 3] per energised case."""
    _fields_ = [("struct_size", C.c_int32), ("nbins", C.c_int32), ("lo", C.c_double * 7), ("hi", C.c_double * 7)]


# numpy dtype with the same layout as amc_path_record
def path_record_dtype():
    import numpy as np
    return np.dtype([("step", "<i4"), ("phase", "<i4"), ("cell", "<i8"), ("i", "<i4"), ("j", "<i4"),
                     ("which", "<i4"), ("reserved", "<i4"), ("total", "<f8"), ("px", "<f8"), ("py", "<f8"),
                     ("pz", "<f8")])


AMC_K_NAMES = ["drift_walls", "bin_count", "bin_scan", "bin_scatter", "detect", "resolve", "bounds", "validate",
               "resolve_more", "commit", "clusters_wide", "fixup", "fields"]
