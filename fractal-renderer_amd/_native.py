"""ctypes loader of libfractal_hip.so (the C ABI of include/fractal_hip.h).

There is no fallback: a missing or unloadable library raises, and every compute call raises
FractalHipError when the HIP path fails (no GPU, HIP error).
"""
import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "libfractal_hip.so")

FR_OK, FR_ERR_INVALID_ARGUMENT, FR_ERR_BUFFER_TOO_SMALL, FR_ERR_NO_DEVICE, FR_ERR_HIP = 0, 1, 2, 3, 4
STATUS_NAMES = {
    1: "FR_ERR_INVALID_ARGUMENT",
    2: "FR_ERR_BUFFER_TOO_SMALL",
    3: "FR_ERR_NO_DEVICE",
    4: "FR_ERR_HIP",
    5: "FR_ERR_UNSUPPORTED_ALGO",
}


class FractalHipError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("%s: %s" % (STATUS_NAMES.get(code, "fr_status %d" % code), message))
        self.code = code


class Imaginary(C.Structure):
    """calc/src/lib.rs:79-82"""

    _fields_ = [("re", C.c_double), ("im", C.c_double)]

    def __iter__(self):
        return iter((self.re, self.im))


class RGB(C.Structure):
    """calc/src/lib.rs:121-125 — the stored fields (see RGB.new for the constructor quirk)."""

    _fields_ = [("r", C.c_uint8), ("g", C.c_uint8), ("b", C.c_uint8)]

    @classmethod
    def new(cls, r, b, g):
        """RGB::new(r, b, g) — calc/src/lib.rs:129-131: the second parameter is BLUE."""
        return cls(r, g, b)

    def __iter__(self):
        return iter((self.r, self.g, self.b))

    def __eq__(self, other):
        return tuple(self) == tuple(other)

    def __repr__(self):
        return "RGB { r: %d, g: %d, b: %d }" % tuple(self)


class fr_config(C.Structure):
    """include/fractal_hip.h fr_config == calc::Config (calc/src/lib.rs:21-37)."""

    _fields_ = [
        ("algo", C.c_uint32),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("iterations", C.c_uint32),
        ("limit", C.c_double),
        ("stable_limit", C.c_double),
        ("pos", Imaginary),
        ("scale", Imaginary),
        ("exposure", C.c_double),
        ("inside", C.c_uint8),
        ("smooth", C.c_uint8),
        ("primary_color", RGB),
        ("secondary_color", RGB),
        ("color_weight", C.c_double),
        ("julia_set", Imaginary),
    ]


class fr_render_opts(C.Structure):
    """include/fractal_hip.h fr_render_opts: the implementation selectors of ONE call."""

    _fields_ = [
        ("size", C.c_uint32),
        ("tile", C.c_int32),
        ("loop_mode", C.c_int32),
        ("palette", C.c_int32),
        ("cycle_shortcut", C.c_int32),
        ("refill_minrun", C.c_int32),
        ("refill_quit16", C.c_int32),
        ("colour_filter", C.c_int32),
    ]


FR_MAX_DEVICES = 16
FR_GATHER_PEER_COPY, FR_GATHER_RCCL = 0, 1


class fr_multi_stats(C.Structure):
    _fields_ = [
        ("n_devices", C.c_uint32),
        ("kernels", C.c_uint32 * FR_MAX_DEVICES),
        ("kernel_ms", C.c_float * FR_MAX_DEVICES),
        ("rows", C.c_uint64 * FR_MAX_DEVICES),
        ("wall_ms", C.c_double),
        ("transfer_span_ms", C.c_float * FR_MAX_DEVICES),
        ("job_ms", C.c_double * FR_MAX_DEVICES),
        ("bytes_moved", C.c_uint64 * FR_MAX_DEVICES),
    ]


class fr_wide_centre(C.Structure):
    """include/fractal_hip.h fr_wide_centre: the view centre of WIDE PT, n_words little-endian uint64 words per axis."""

    _fields_ = [("n_words", C.c_uint32), ("re", C.POINTER(C.c_uint64)), ("im", C.POINTER(C.c_uint64))]


FR_STATS_BINS = 1024


class fr_view_stats(C.Structure):
    """include/fractal_hip.h fr_view_stats: the escape-index statistics of a kept view (sizeof == 8248)."""

    _fields_ = [
        ("n", C.c_uint64),
        ("stable", C.c_uint64),
        ("capped", C.c_uint64),
        ("escaped", C.c_uint64),
        ("sum_iters", C.c_uint64),
        ("min_iters", C.c_uint32),
        ("max_iters", C.c_uint32),
        ("shift", C.c_uint32),
        ("reserved", C.c_uint32),
        ("hist", C.c_uint64 * FR_STATS_BINS),
    ]


FR_WIDE_MAX_WORDS = 16
FR_BLA_DEFAULT_BITS = 40
FR_PT_ROAD_PLAIN, FR_PT_ROAD_BLA, FR_PT_ROAD_SCALED = 0, 1, 2  # fr_pt_road
_OPTS = C.POINTER(fr_render_opts)
_WIDE = C.POINTER(fr_wide_centre)

# name -> (restype, argtypes); every symbol include/fractal_hip.h declares
PROTOTYPES = {
    "fr_abi_version": (C.c_int, []),
    "fr_build_id": (C.c_char_p, []),
    "fr_render_opts_init": (None, [_OPTS]),
    "fr_render_rows_rgb8_device_opts": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, _OPTS],
    ),
    "fr_render_rows_rgba8_device_opts": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, _OPTS],
    ),
    "fr_render_rows_rgb8_opts": (
        C.c_int, [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, _OPTS]),
    "fr_render_block_cyclic_range_rgb8_device_opts": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t,
         C.c_void_p, C.POINTER(C.c_uint64), _OPTS],
    ),
    "fr_render_fern_rgb8": (C.c_int, [C.POINTER(fr_config), C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.c_size_t]),
    "fr_init_devices": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "fr_multi_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "fr_set_multi_root_share": (C.c_int, [C.c_int]),
    "fr_render_rgb8_multi": (C.c_int, [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_void_p, C.c_size_t]),
    "fr_render_rgb8_multi_device": (
        C.c_int, [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t]),
    "fr_multi_last_stats": (C.c_int, [C.POINTER(fr_multi_stats)]),
    "fr_debug_rccl_selftest": (C.c_int, [C.c_size_t]),
    "fr_debug_rccl_probe": (C.c_int, []),
    "fr_set_dispatch_sampling": (C.c_int, [C.c_int]),
    "fr_debug_sample_view": (C.c_int, [C.POINTER(fr_config), C.c_int, C.POINTER(C.c_double)]),
    "fr_debug_view_choice": (C.c_int, [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_int),
                                       C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "fr_debug_inject_multi_failure": (C.c_int, [C.c_int, C.c_int]),
    "fr_pin_host_buffer": (C.c_int, [C.c_void_p, C.c_size_t]),
    "fr_unpin_host_buffer": (C.c_int, [C.c_void_p]),
    "fr_last_kernel_name": (C.c_int, [C.c_char_p, C.c_size_t]),
    "fr_set_colour_filter": (C.c_int, [C.c_int]),
    "fr_init": (C.c_int, [C.c_int]),
    "fr_shutdown": (C.c_int, []),
    "fr_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "fr_device_name": (C.c_int, [C.c_char_p, C.c_size_t]),
    "fr_last_error": (C.c_char_p, []),
    "fr_config_new": (None, [C.POINTER(fr_config), C.c_uint32]),
    "fr_render_rgb8": (C.c_int, [C.POINTER(fr_config), C.c_void_p, C.c_size_t]),
    "fr_render_rows_rgb8": (C.c_int, [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]),
    "fr_render_rows_rgb8_device": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p],
    ),
    "fr_render_rows_rgba8": (C.c_int, [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]),
    "fr_render_rows_rgba8_device": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p],
    ),
    "fr_render_block_cyclic_rgb8_device": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
         C.POINTER(C.c_uint64)],
    ),
    "fr_render_block_cyclic_range_rgb8_device": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t,
         C.c_void_p, C.POINTER(C.c_uint64)],
    ),
    "fr_render_block_cyclic_rgb8": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
         C.POINTER(C.c_uint64)],
    ),
    "fr_block_cyclic_rows": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "fr_pixel": (C.c_int, [C.POINTER(fr_config), C.c_uint32, C.c_uint32, C.POINTER(RGB)]),
    "fr_pixel_p": (C.c_int, [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.POINTER(RGB)]),
    "fr_recursive": (
        C.c_int,
        [C.c_uint32, Imaginary, Imaginary, C.c_double, C.POINTER(Imaginary), C.POINTER(C.c_uint32)],
    ),
    "fr_recursive_batch": (
        C.c_int,
        [C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_void_p, C.c_void_p],
    ),
    "fr_escape_rows": (C.c_int, [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "fr_render_rows_dd": (
        C.c_int, [C.POINTER(fr_config), C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t]),
    "fr_render_rows_dd_device": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p],
    ),
    "fr_escape_rows_dd": (
        C.c_int, [C.POINTER(fr_config), C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "fr_render_rows_pt": (
        C.c_int, [C.POINTER(fr_config), C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t]),
    "fr_render_rows_pt_device": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p],
    ),
    "fr_escape_rows_pt": (
        C.c_int, [C.POINTER(fr_config), C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "fr_debug_reference_orbit": (
        C.c_int, [C.POINTER(fr_config), C.POINTER(Imaginary), C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]),
    "fr_ss_workspace_bytes": (
        C.c_int, [C.POINTER(fr_config), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "fr_render_rows_ss_device": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p,
         C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, _OPTS],
    ),
    "fr_render_rows_ss": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p,
         C.c_size_t, _OPTS],
    ),
    "fr_box_filter_rgb8": (
        C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t]),
    "fr_box_filter_rgb8_device": (
        C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "fr_colour_rgb8": (C.c_int, [C.POINTER(fr_config), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "fr_colour_rgb8_device": (
        C.c_int, [C.POINTER(fr_config), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "fr_escape_rows_device": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
         C.c_void_p, _OPTS],
    ),
    "fr_escape_extend_device": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p,
         C.c_void_p, C.c_void_p, _OPTS],
    ),
    "fr_escape_extend": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p,
         C.c_void_p],
    ),
    "fr_escape_rows_pt_state_device": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
         C.c_void_p],
    ),
    "fr_escape_extend_pt_device": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
         C.c_void_p, C.c_void_p],
    ),
    "fr_escape_rows_pt_state": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "fr_escape_extend_pt": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
         C.c_void_p],
    ),
    "fr_debug_pt_orbit_cache": (C.c_int, [C.POINTER(C.c_uint32)]),
    "fr_wide_from_double": (C.c_int, [C.c_double, C.c_void_p, C.c_uint32]),
    "fr_wide_add_double": (C.c_int, [C.c_void_p, C.c_uint32, C.c_double]),
    "fr_wide_to_double": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "fr_wide_from_decimal": (C.c_int, [C.c_char_p, C.c_void_p, C.c_uint32]),
    "fr_render_rows_pt_wide": (
        C.c_int, [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t]),
    "fr_render_rows_pt_wide_device": (
        C.c_int, [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "fr_escape_rows_pt_wide": (C.c_int, [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "fr_escape_rows_pt_wide_state_device": (
        C.c_int,
        [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "fr_escape_extend_pt_wide_device": (
        C.c_int,
        [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
         C.c_void_p],
    ),
    "fr_escape_rows_pt_wide_state": (
        C.c_int, [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fr_escape_extend_pt_wide": (
        C.c_int,
        [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "fr_debug_reference_orbit_wide": (
        C.c_int, [C.POINTER(fr_config), _WIDE, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]),
    "fr_render_rows_pt_bla": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), _WIDE, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t]),
    "fr_render_rows_pt_bla_device": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), _WIDE, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t,
         C.c_void_p],
    ),
    "fr_escape_rows_pt_bla": (
        C.c_int, [C.POINTER(fr_config), C.POINTER(Imaginary), _WIDE, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "fr_escape_rows_pt_bla_device": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), _WIDE, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "fr_debug_bla_table": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), _WIDE, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t,
         C.POINTER(C.c_uint32)],
    ),
    "fr_debug_bla_count": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), _WIDE, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64),
         C.POINTER(C.c_uint64)],
    ),
    "fr_debug_bla_cache": (C.c_int, [C.POINTER(C.c_uint32)]),
    "fr_render_rows_pt_scaled": (
        C.c_int, [C.POINTER(fr_config), _WIDE, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t]),
    "fr_render_rows_pt_scaled_device": (
        C.c_int, [C.POINTER(fr_config), _WIDE, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "fr_escape_rows_pt_scaled": (C.c_int, [C.POINTER(fr_config), _WIDE, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "fr_escape_rows_pt_scaled_device": (
        C.c_int, [C.POINTER(fr_config), _WIDE, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fr_debug_bla_table_scaled": (
        C.c_int, [C.POINTER(fr_config), _WIDE, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]),
    "fr_debug_pt_scaled_count": (
        C.c_int, [C.POINTER(fr_config), _WIDE, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fr_escape_rows_pt_scaled_state_device": (
        C.c_int,
        [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "fr_escape_extend_pt_scaled_device": (
        C.c_int,
        [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
         C.c_void_p],
    ),
    "fr_escape_rows_pt_scaled_state": (
        C.c_int, [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fr_escape_extend_pt_scaled": (
        C.c_int,
        [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "fr_render_rows_ss_pt_device": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), _WIDE, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
         C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p],
    ),
    "fr_render_rows_ss_pt": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), _WIDE, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
         C.c_void_p, C.c_size_t],
    ),
    "fr_colour_rows_ss_device": (
        C.c_int,
        [C.POINTER(fr_config), C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p,
         C.c_size_t, C.c_void_p],
    ),
    "fr_colour_ss_rgb8": (
        C.c_int,
        [C.POINTER(fr_config), C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p,
         C.c_size_t],
    ),
    "fr_colour_rows_device": (
        C.c_int,
        [C.POINTER(fr_config), C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p],
    ),
    "fr_view_stats_device": (
        C.c_int, [C.POINTER(fr_config), C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "fr_view_stats": (C.c_int, [C.POINTER(fr_config), C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(fr_view_stats)]),
    "fr_stats_percentile": (C.c_int, [C.POINTER(fr_view_stats), C.c_double, C.POINTER(C.c_uint32)]),
    "fr_auto_exposure": (C.c_int, [C.POINTER(fr_config), C.POINTER(fr_view_stats), C.c_double, C.POINTER(C.c_double)]),
    "fr_escape_rows_de_device": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "fr_escape_rows_de": (
        C.c_int, [C.POINTER(fr_config), C.c_int, C.POINTER(Imaginary), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fr_escape_rows_de_pt_wide_device": (
        C.c_int, [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fr_escape_rows_de_pt_wide": (
        C.c_int, [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fr_escape_rows_de_pt_bla_device": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), _WIDE, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
         C.c_void_p],
    ),
    "fr_escape_rows_de_pt_bla": (
        C.c_int, [C.POINTER(fr_config), C.POINTER(Imaginary), _WIDE, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fr_escape_rows_de_pt_scaled_device": (
        C.c_int, [C.POINTER(fr_config), _WIDE, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fr_escape_rows_de_pt_scaled": (
        C.c_int, [C.POINTER(fr_config), _WIDE, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fr_de_scaled_view": (C.c_int, [C.POINTER(fr_config), C.POINTER(fr_config)]),
    "fr_escape_extend_de_device": (
        C.c_int, [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fr_escape_extend_de": (
        C.c_int, [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fr_escape_rows_de_pt_state_device": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), _WIDE, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
         C.c_void_p, C.c_void_p],
    ),
    "fr_escape_rows_de_pt_state": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), _WIDE, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
         C.c_void_p],
    ),
    "fr_escape_extend_de_pt_device": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), _WIDE, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
         C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "fr_escape_extend_de_pt": (
        C.c_int,
        [C.POINTER(fr_config), C.POINTER(Imaginary), _WIDE, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
         C.c_void_p, C.c_void_p],
    ),
    "fr_escape_rows_de_pt_scaled_state_device": (
        C.c_int,
        [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "fr_escape_rows_de_pt_scaled_state": (
        C.c_int, [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fr_escape_extend_de_pt_scaled_device": (
        C.c_int,
        [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
         C.c_void_p],
    ),
    "fr_escape_extend_de_pt_scaled": (
        C.c_int,
        [C.POINTER(fr_config), _WIDE, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    ),
    "fr_distance_rows_device": (
        C.c_int, [C.POINTER(fr_config), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "fr_distance_rows": (C.c_int, [C.POINTER(fr_config), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "fr_colour_de_rows_device": (
        C.c_int,
        [C.POINTER(fr_config), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_void_p, C.c_void_p],
    ),
    "fr_colour_de_rgb8": (
        C.c_int, [C.POINTER(fr_config), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_size_t]),
    "fr_colour_de_rows_ss_device": (
        C.c_int,
        [C.POINTER(fr_config), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_void_p,
         C.c_size_t, C.c_void_p],
    ),
    "fr_colour_de_ss_rgb8": (
        C.c_int,
        [C.POINTER(fr_config), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_void_p,
         C.c_size_t],
    ),
    "fr_ss_de_workspace_bytes": (
        C.c_int, [C.POINTER(fr_config), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "fr_render_rows_ss_de_device": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.POINTER(Imaginary), _WIDE, C.c_int, C.c_int, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32,
         C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p],
    ),
    "fr_render_rows_ss_de": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.POINTER(Imaginary), _WIDE, C.c_int, C.c_int, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32,
         C.c_int, C.c_void_p, C.c_size_t],
    ),
    "fr_render_rows_ss_de_pt_scaled_device": (
        C.c_int,
        [C.POINTER(fr_config), _WIDE, C.c_int, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t,
         C.c_void_p, C.c_size_t, C.c_void_p],
    ),
    "fr_render_rows_ss_de_pt_scaled": (
        C.c_int,
        [C.POINTER(fr_config), _WIDE, C.c_int, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t],
    ),
    "fr_ss_adaptive_workspace_bytes": (
        C.c_int, [C.POINTER(fr_config), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t)]),
    "fr_render_rows_ss_adaptive_device": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.POINTER(Imaginary), _WIDE, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
         C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p],
    ),
    "fr_render_rows_ss_adaptive": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.POINTER(Imaginary), _WIDE, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
         C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)],
    ),
    "fr_debug_ss_adaptive_grid": (C.c_int, [C.c_uint32]),
    "fr_debug_ss_host_work_cap": (C.c_int, [C.c_size_t]),
    "fr_ss_adaptive_de_workspace_bytes": (
        C.c_int, [C.POINTER(fr_config), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t)]),
    "fr_render_rows_ss_adaptive_de_device": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.POINTER(Imaginary), _WIDE, C.c_int, C.c_int, C.c_double, C.c_uint32, C.c_int, C.c_double,
         C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p],
    ),
    "fr_render_rows_ss_adaptive_de": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.POINTER(Imaginary), _WIDE, C.c_int, C.c_int, C.c_double, C.c_uint32, C.c_int, C.c_double,
         C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)],
    ),
    "fr_render_rows_ss_adaptive_de_pt_scaled_device": (
        C.c_int,
        [C.POINTER(fr_config), _WIDE, C.c_int, C.c_double, C.c_uint32, C.c_int, C.c_double, C.c_uint32, C.c_uint32, C.c_int,
         C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p],
    ),
    "fr_render_rows_ss_adaptive_de_pt_scaled": (
        C.c_int,
        [C.POINTER(fr_config), _WIDE, C.c_int, C.c_double, C.c_uint32, C.c_int, C.c_double, C.c_uint32, C.c_uint32, C.c_int,
         C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)],
    ),
    "fr_count_iterations": (
        C.c_int,
        [C.POINTER(fr_config), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64),
         C.POINTER(C.c_uint64)],
    ),
    "fr_set_profiling": (C.c_int, [C.c_int]),
    "fr_last_kernel_ms": (C.c_int, [C.POINTER(C.c_float)]),
    "fr_set_tile": (C.c_int, [C.c_int]),
    "fr_set_loop_mode": (C.c_int, [C.c_int]),
    "fr_debug_loop_plan": (C.c_int, [C.POINTER(fr_config), C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_double),
                                     C.POINTER(C.c_uint32)]),
    "fr_debug_set_spec_maxlen": (C.c_int, [C.c_uint32]),
    "fr_debug_spec_maxlen": (C.c_int, [C.POINTER(fr_config), C.c_int, C.POINTER(C.c_uint32)]),
    "fr_set_palette": (C.c_int, [C.c_int]),
    "fr_set_cycle_shortcut": (C.c_int, [C.c_int]),
    "fr_set_refill_policy": (C.c_int, [C.c_int, C.c_int]),
    "fr_debug_math": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "fr_debug_set_queue_trace": (C.c_int, [C.c_void_p]),
    "fr_debug_set_two_pass_capacity": (C.c_int, [C.c_uint32]),
}

# LINEAR-LIGHT SUPERSAMPLING: every _tf call is its twin with `int transfer` behind `supersample`, whose index is given here
_TF_TWINS = {
    "fr_box_filter_rgb8": 3, "fr_box_filter_rgb8_device": 3,
    "fr_render_rows_ss": 3, "fr_render_rows_ss_device": 3,
    "fr_render_rows_ss_pt": 5, "fr_render_rows_ss_pt_device": 5,
    "fr_colour_rows_ss_device": 6, "fr_colour_ss_rgb8": 6,
    "fr_colour_de_rows_ss_device": 6, "fr_colour_de_ss_rgb8": 6,
    "fr_render_rows_ss_de": 7, "fr_render_rows_ss_de_device": 7,
    "fr_render_rows_ss_de_pt_scaled": 4, "fr_render_rows_ss_de_pt_scaled_device": 4,
    "fr_render_rows_ss_adaptive": 6, "fr_render_rows_ss_adaptive_device": 6,
    "fr_render_rows_ss_adaptive_de": 7, "fr_render_rows_ss_adaptive_de_device": 7,
}


def tf_name(twin):
    """fr_x -> fr_x_tf, fr_x_device -> fr_x_tf_device."""
    return twin[:-len("_device")] + "_tf_device" if twin.endswith("_device") else twin + "_tf"


for _twin, _k in _TF_TWINS.items():
    _res, _args = PROTOTYPES[_twin]
    assert _args[_k] is C.c_uint32
    PROTOTYPES[tf_name(_twin)] = (_res, _args[:_k + 1] + [C.c_int] + _args[_k + 1:])
# ADAPTIVE SUPERSAMPLED SCALED DE's twins, by the same rule: `int transfer` behind `supersample` (argument 4)
for _twin in ("fr_render_rows_ss_adaptive_de_pt_scaled", "fr_render_rows_ss_adaptive_de_pt_scaled_device"):
    _res, _args = PROTOTYPES[_twin]
    assert _args[4] is C.c_uint32
    PROTOTYPES[tf_name(_twin)] = (_res, _args[:5] + [C.c_int] + _args[5:])
PROTOTYPES["fr_ss_transfer_tables"] = (C.c_int, [C.POINTER(C.POINTER(C.c_uint16)), C.POINTER(C.POINTER(C.c_uint16))])

_lib = None


def load():
    """Load libfractal_hip.so and bind every prototype.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing — build it first (python -c 'import __graft_entry__ as g; g.build()'); "
            "this package has no CPU fallback" % LIB_PATH
        )
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI lost a symbol
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(rc):
    if rc != FR_OK:
        msg = load().fr_last_error()
        raise FractalHipError(rc, msg.decode() if msg else "")
