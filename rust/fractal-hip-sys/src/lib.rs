//! `extern "C"` bindings to libfractal_hip.so (include/fractal_hip.h) plus the safe wrappers the
//! reference's `get_image` / `get_recursive_pixel` / `recursive` call sites need.
//!
//! The `#[repr(C)]` types are the C ABI's image of `calc::Config`, `calc::Imaginary` and
//! `calc::RGB` (calc/src/lib.rs:21-37, 79-82, 121-125).  `calc::RGB` is `repr(Rust)` today although
//! the reference already transmutes it to 3 packed bytes (src/lib.rs:13-15, src/gui.rs:62-64);
//! adding `#[repr(C)]` to it makes that assumption sound and lets `Vec<RGB>` be filled in place.
//!
//! Untested in this pipeline (no rustc); kept mechanical on purpose.
#![allow(non_camel_case_types)]

use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct fr_imaginary {
    pub re: f64,
    pub im: f64,
}

/// The STORED fields of `calc::RGB` (not `RGB::new`'s `(r, b, g)` parameter order).
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct fr_rgb {
    pub r: u8,
    pub g: u8,
    pub b: u8,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fr_config {
    pub algo: u32, // 0 Mandelbrot, 1 BarnsleyFern, 2 Julia (calc/src/lib.rs:150-154)
    pub width: u32,
    pub height: u32,
    pub iterations: u32,
    pub limit: f64,
    pub stable_limit: f64,
    pub pos: fr_imaginary,
    pub scale: fr_imaginary,
    pub exposure: f64,
    pub inside: u8,
    pub smooth: u8,
    pub primary_color: fr_rgb,
    pub secondary_color: fr_rgb,
    pub color_weight: f64,
    pub julia_set: fr_imaginary,
}

/// The implementation selectors of ONE call (include/fractal_hip.h, `fr_render_opts`); fill with `fr_render_opts_init`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fr_render_opts {
    pub size: u32,
    pub tile: i32,
    pub loop_mode: i32,
    pub palette: i32,
    pub cycle_shortcut: i32,
    pub refill_minrun: i32,
    pub refill_quit16: i32,
    pub colour_filter: i32,
}

/// The view centre of WIDE PT (include/fractal_hip.h, "WIDE PT"): `n_words` little-endian words per axis, two's complement,
/// value `I / 2^(64 n_words - 8)`.  The caller owns the words.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct fr_wide_centre {
    pub n_words: u32,
    pub re: *const u64,
    pub im: *const u64,
}

pub const FR_OK: c_int = 0;
/// Largest word count of a wide centre.
pub const FR_WIDE_MAX_WORDS: u32 = 16;
/// Largest `supersample` of the supersampled renders (include/fractal_hip.h, "supersampled rendering").
pub const FR_SS_MAX: u32 = 8;
/// `FR_ABI_VERSION` of the header these declarations were written against; `check_abi()` compares it with the library's.
pub const FR_ABI_VERSION: c_int = 3;
pub const FR_PRECISION_F64: c_int = 0;
pub const FR_PRECISION_F32: c_int = 1;
/// Double-double (~106-bit) arithmetic for zooms past the f64 limit (include/fractal_hip.h, `fr_precision`).
pub const FR_PRECISION_DD: c_int = 2;
/// Perturbation: one double-double reference orbit per view, f64 offsets per pixel (include/fractal_hip.h, `fr_precision`).
pub const FR_PRECISION_PT: c_int = 3;

extern "C" {
    pub fn fr_init(device: c_int) -> c_int;
    pub fn fr_shutdown() -> c_int;
    pub fn fr_device_count(count: *mut c_int) -> c_int;
    pub fn fr_last_error() -> *const c_char;
    pub fn fr_abi_version() -> c_int;
    pub fn fr_build_id() -> *const c_char;
    pub fn fr_device_name(buf: *mut c_char, buf_len: usize) -> c_int;
    pub fn fr_config_new(cfg: *mut fr_config, algo: u32);
    pub fn fr_render_rgb8(cfg: *const fr_config, out: *mut u8, out_len: usize) -> c_int;
    pub fn fr_render_rows_rgb8(cfg: *const fr_config, precision: c_int, y0: u32, y1: u32, out: *mut u8, out_len: usize) -> c_int;
    pub fn fr_render_rows_rgb8_device(cfg: *const fr_config, precision: c_int, y0: u32, y1: u32, d_out: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    pub fn fr_render_rows_rgba8(cfg: *const fr_config, precision: c_int, y0: u32, y1: u32, out: *mut u8, out_len: usize) -> c_int;
    pub fn fr_render_rows_rgba8_device(cfg: *const fr_config, precision: c_int, y0: u32, y1: u32, d_out: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    pub fn fr_pixel(cfg: *const fr_config, x: u32, y: u32, out: *mut fr_rgb) -> c_int;
    pub fn fr_pixel_p(cfg: *const fr_config, precision: c_int, x: u32, y: u32, out: *mut fr_rgb) -> c_int;
    pub fn fr_recursive(iterations: u32, start: fr_imaginary, c: fr_imaginary, limit: f64, out_pos: *mut fr_imaginary, out_iters: *mut u32) -> c_int;
    pub fn fr_recursive_batch(iterations: u32, start: *const fr_imaginary, c: *const fr_imaginary, n: usize, limit: f64, precision: c_int, out_pos: *mut fr_imaginary, out_iters: *mut u32) -> c_int;
    pub fn fr_escape_rows(cfg: *const fr_config, precision: c_int, y0: u32, y1: u32, z_re_im: *mut f64, iters: *mut u32) -> c_int;
    // the colour map alone over stored recursive() results: what the GUI's exposure / colour controls need (src/gui.rs:183-203)
    pub fn fr_colour_rgb8(cfg: *const fr_config, z_re_im: *const f64, iters: *const u32, n: usize, out: *mut u8, out_len: usize) -> c_int;
    // one process, several GPUs (include/fractal_hip.h, "get_image across several GPUs from ONE process")
    pub fn fr_init_devices(devices: *const c_int, n: c_int) -> c_int;
    pub fn fr_render_rgb8_multi(cfg: *const fr_config, precision: c_int, block_rows: u32, out: *mut u8, out_len: usize) -> c_int;
    // a frame buffer that is rendered into again and again: pin it once; unpin before freeing it
    pub fn fr_pin_host_buffer(ptr: *mut c_void, len: usize) -> c_int;
    pub fn fr_unpin_host_buffer(ptr: *mut c_void) -> c_int;
    // the default dispatch's view sample (blocking only in front of the first launch of a view of 4096 x 2048 pixels and more): 0 = off
    pub fn fr_set_dispatch_sampling(enabled: c_int) -> c_int;
    // Algo::BarnsleyFern (src/lib.rs:271-319, 417-463) on the GPU
    pub fn fr_render_fern_rgb8(cfg: *const fr_config, threads: u32, seed: u64, walkers: u32, out: *mut u8, out_len: usize) -> c_int;
    // deep zoom: FR_PRECISION_DD with the low halves of the view centre (NULL = (0, 0))
    pub fn fr_render_rows_dd(cfg: *const fr_config, pos_lo: *const fr_imaginary, y0: u32, y1: u32, channels: c_int, out: *mut u8, out_len: usize) -> c_int;
    pub fn fr_render_rows_dd_device(cfg: *const fr_config, pos_lo: *const fr_imaginary, y0: u32, y1: u32, channels: c_int, d_out: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    pub fn fr_escape_rows_dd(cfg: *const fr_config, pos_lo: *const fr_imaginary, y0: u32, y1: u32, z: *mut f64, iters: *mut u32) -> c_int;
    // deep zoom: FR_PRECISION_PT (perturbation) with the low halves of the view centre (NULL = (0, 0))
    pub fn fr_render_rows_pt(cfg: *const fr_config, pos_lo: *const fr_imaginary, y0: u32, y1: u32, channels: c_int, out: *mut u8, out_len: usize) -> c_int;
    pub fn fr_render_rows_pt_device(cfg: *const fr_config, pos_lo: *const fr_imaginary, y0: u32, y1: u32, channels: c_int, d_out: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    pub fn fr_escape_rows_pt(cfg: *const fr_config, pos_lo: *const fr_imaginary, y0: u32, y1: u32, z: *mut f64, iters: *mut u32) -> c_int;
    // supersampled rendering: render `supersample` times as large, box-filter on the device (pos_lo NULL unless DD / PT; opts NULL = defaults)
    pub fn fr_ss_workspace_bytes(cfg: *const fr_config, supersample: u32, y0: u32, y1: u32, min_bytes: *mut usize, best_bytes: *mut usize) -> c_int;
    pub fn fr_render_rows_ss_device(cfg: *const fr_config, precision: c_int, pos_lo: *const fr_imaginary, supersample: u32, y0: u32, y1: u32, channels: c_int, d_out: *mut c_void, out_len: usize, d_work: *mut c_void, work_len: usize, hip_stream: *mut c_void, opts: *const fr_render_opts) -> c_int;
    pub fn fr_render_rows_ss(cfg: *const fr_config, precision: c_int, pos_lo: *const fr_imaginary, supersample: u32, y0: u32, y1: u32, channels: c_int, out: *mut u8, out_len: usize, opts: *const fr_render_opts) -> c_int;
    pub fn fr_box_filter_rgb8(src: *const u8, width: u32, rows: u32, supersample: u32, channels: c_int, out: *mut u8, out_len: usize) -> c_int;
    pub fn fr_box_filter_rgb8_device(d_src: *const c_void, width: u32, rows: u32, supersample: u32, channels: c_int, d_out: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    // a view kept on the device (include/fractal_hip.h): raw results into device arrays, their cap raised in place, the colour map over them
    pub fn fr_escape_rows_device(cfg: *const fr_config, precision: c_int, pos_lo: *const fr_imaginary, y0: u32, y1: u32, z_width: c_int, d_z: *mut c_void, d_iters: *mut c_void, hip_stream: *mut c_void, opts: *const fr_render_opts) -> c_int;
    pub fn fr_escape_extend_device(cfg: *const fr_config, precision: c_int, pos_lo: *const fr_imaginary, y0: u32, y1: u32, from_iterations: u32, z_width: c_int, d_z: *mut c_void, d_iters: *mut c_void, hip_stream: *mut c_void, opts: *const fr_render_opts) -> c_int;
    pub fn fr_escape_extend(cfg: *const fr_config, precision: c_int, pos_lo: *const fr_imaginary, y0: u32, y1: u32, from_iterations: u32, z_width: c_int, z: *mut f64, iters: *mut u32) -> c_int;
    pub fn fr_colour_rows_device(cfg: *const fr_config, d_z: *const c_void, z_width: c_int, d_iters: *const c_void, n: usize, channels: c_int, d_out: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    // resumable perturbation (include/fractal_hip.h): a PT view's state (z, iters, dz, m) and its cap raised in place
    pub fn fr_escape_rows_pt_state_device(cfg: *const fr_config, pos_lo: *const fr_imaginary, y0: u32, y1: u32, d_z: *mut c_void, d_iters: *mut c_void, d_dz: *mut c_void, d_m: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn fr_escape_extend_pt_device(cfg: *const fr_config, pos_lo: *const fr_imaginary, y0: u32, y1: u32, from_iterations: u32, d_z: *mut c_void, d_iters: *mut c_void, d_dz: *mut c_void, d_m: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn fr_escape_rows_pt_state(cfg: *const fr_config, pos_lo: *const fr_imaginary, y0: u32, y1: u32, z: *mut f64, iters: *mut u32, dz: *mut f64, m: *mut u32) -> c_int;
    pub fn fr_escape_extend_pt(cfg: *const fr_config, pos_lo: *const fr_imaginary, y0: u32, y1: u32, from_iterations: u32, z: *mut f64, iters: *mut u32, dz: *mut f64, m: *mut u32) -> c_int;
    // WIDE PT (include/fractal_hip.h): a fixed-point view centre of up to 1016 bits; the helpers are host only
    pub fn fr_wide_from_double(v: f64, w: *mut u64, n: u32) -> c_int;
    pub fn fr_wide_add_double(w: *mut u64, n: u32, delta: f64) -> c_int;
    pub fn fr_wide_to_double(w: *const u64, n: u32, hi: *mut f64, lo: *mut f64) -> c_int;
    pub fn fr_wide_from_decimal(text: *const c_char, w: *mut u64, n: u32) -> c_int;
    pub fn fr_render_rows_pt_wide(cfg: *const fr_config, centre: *const fr_wide_centre, y0: u32, y1: u32, channels: c_int, out: *mut u8, out_len: usize) -> c_int;
    pub fn fr_render_rows_pt_wide_device(cfg: *const fr_config, centre: *const fr_wide_centre, y0: u32, y1: u32, channels: c_int, d_out: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    pub fn fr_escape_rows_pt_wide(cfg: *const fr_config, centre: *const fr_wide_centre, y0: u32, y1: u32, z: *mut f64, iters: *mut u32) -> c_int;
    pub fn fr_escape_rows_pt_wide_state_device(cfg: *const fr_config, centre: *const fr_wide_centre, y0: u32, y1: u32, d_z: *mut c_void, d_iters: *mut c_void, d_dz: *mut c_void, d_m: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn fr_escape_extend_pt_wide_device(cfg: *const fr_config, centre: *const fr_wide_centre, y0: u32, y1: u32, from_iterations: u32, d_z: *mut c_void, d_iters: *mut c_void, d_dz: *mut c_void, d_m: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn fr_escape_rows_pt_wide_state(cfg: *const fr_config, centre: *const fr_wide_centre, y0: u32, y1: u32, z: *mut f64, iters: *mut u32, dz: *mut f64, m: *mut u32) -> c_int;
    pub fn fr_escape_extend_pt_wide(cfg: *const fr_config, centre: *const fr_wide_centre, y0: u32, y1: u32, from_iterations: u32, z: *mut f64, iters: *mut u32, dz: *mut f64, m: *mut u32) -> c_int;
    pub fn fr_debug_reference_orbit_wide(cfg: *const fr_config, centre: *const fr_wide_centre, which: c_int, out: *mut f64, cap: usize, len: *mut u32) -> c_int;
    // BLA-PT (include/fractal_hip.h): perturbation that skips iterations in bulk; centre non-null selects the wide road (pos_lo null then)
    pub fn fr_render_rows_pt_bla(cfg: *const fr_config, pos_lo: *const fr_imaginary, centre: *const fr_wide_centre, bits: c_int, y0: u32, y1: u32, channels: c_int, out: *mut u8, out_len: usize) -> c_int;
    pub fn fr_render_rows_pt_bla_device(cfg: *const fr_config, pos_lo: *const fr_imaginary, centre: *const fr_wide_centre, bits: c_int, y0: u32, y1: u32, channels: c_int, d_out: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    pub fn fr_escape_rows_pt_bla(cfg: *const fr_config, pos_lo: *const fr_imaginary, centre: *const fr_wide_centre, bits: c_int, y0: u32, y1: u32, z: *mut f64, iters: *mut u32) -> c_int;
    pub fn fr_escape_rows_pt_bla_device(cfg: *const fr_config, pos_lo: *const fr_imaginary, centre: *const fr_wide_centre, bits: c_int, y0: u32, y1: u32, d_z: *mut c_void, d_iters: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn fr_debug_bla_table(cfg: *const fr_config, pos_lo: *const fr_imaginary, centre: *const fr_wide_centre, bits: c_int, which: c_int, level: u32, out: *mut f64, cap: usize, len: *mut u32) -> c_int;
    pub fn fr_debug_bla_count(cfg: *const fr_config, pos_lo: *const fr_imaginary, centre: *const fr_wide_centre, bits: c_int, y0: u32, y1: u32, passes: *mut u64, steps: *mut u64) -> c_int;
    pub fn fr_debug_bla_cache(out: *mut u32) -> c_int;
    pub fn fr_render_rows_pt_scaled(cfg: *const fr_config, centre: *const fr_wide_centre, bits: c_int, y0: u32, y1: u32, channels: c_int, out: *mut u8, out_len: usize) -> c_int;
    pub fn fr_render_rows_pt_scaled_device(cfg: *const fr_config, centre: *const fr_wide_centre, bits: c_int, y0: u32, y1: u32, channels: c_int, d_out: *mut c_void, out_len: usize, hip_stream: *mut c_void) -> c_int;
    pub fn fr_escape_rows_pt_scaled(cfg: *const fr_config, centre: *const fr_wide_centre, bits: c_int, y0: u32, y1: u32, z: *mut f64, iters: *mut u32) -> c_int;
    pub fn fr_escape_rows_pt_scaled_device(cfg: *const fr_config, centre: *const fr_wide_centre, bits: c_int, y0: u32, y1: u32, d_z: *mut c_void, d_iters: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn fr_debug_bla_table_scaled(cfg: *const fr_config, centre: *const fr_wide_centre, bits: c_int, which: c_int, level: u32, out: *mut f64, cap: usize, len: *mut u32) -> c_int;
    pub fn fr_debug_pt_scaled_count(cfg: *const fr_config, centre: *const fr_wide_centre, bits: c_int, y0: u32, y1: u32, passes: *mut u64, steps: *mut u64) -> c_int;
    pub fn fr_escape_rows_pt_scaled_state_device(cfg: *const fr_config, centre: *const fr_wide_centre, y0: u32, y1: u32, d_z: *mut c_void, d_iters: *mut c_void, d_w: *mut c_void, d_m: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn fr_escape_extend_pt_scaled_device(cfg: *const fr_config, centre: *const fr_wide_centre, y0: u32, y1: u32, from_iterations: u32, d_z: *mut c_void, d_iters: *mut c_void, d_w: *mut c_void, d_m: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn fr_escape_rows_pt_scaled_state(cfg: *const fr_config, centre: *const fr_wide_centre, y0: u32, y1: u32, z: *mut f64, iters: *mut u32, w: *mut f64, m: *mut u32) -> c_int;
    pub fn fr_escape_extend_pt_scaled(cfg: *const fr_config, centre: *const fr_wide_centre, y0: u32, y1: u32, from_iterations: u32, z: *mut f64, iters: *mut u32, w: *mut f64, m: *mut u32) -> c_int;
}

/// Message of the last failing call on this thread.
pub fn last_error() -> String {
    unsafe {
        let p = fr_last_error();
        if p.is_null() { String::new() } else { CStr::from_ptr(p).to_string_lossy().into_owned() }
    }
}

/// Select the GPUs `render_into` spreads an image over (row-block-cyclically, one host thread and one
/// PCIe link per GPU).  Not calling it, or passing one device, renders on a single GPU.
pub fn use_devices(devices: &[c_int]) -> Result<(), String> {
    let rc = unsafe { fr_init_devices(devices.as_ptr(), devices.len() as c_int) };
    if rc != FR_OK { Err(last_error()) } else { MULTI.store(devices.len() > 1, std::sync::atomic::Ordering::Relaxed); Ok(()) }
}
static MULTI: std::sync::atomic::AtomicBool = std::sync::atomic::AtomicBool::new(false);

/// `get_image` for `Algo::Mandelbrot | Algo::Julia` (src/lib.rs:253-270): fills a caller-owned
/// pixel vector in place.  `P` must be a 3-byte `#[repr(C)]` pixel (`calc::RGB` once annotated).
pub fn render_into<P: Copy>(cfg: &fr_config, image: &mut Vec<P>) -> Result<(), String> {
    assert_eq!(std::mem::size_of::<P>(), 3, "pixel type must be 3 packed bytes");
    let n = cfg.width as usize * cfg.height as usize;
    image.clear();
    image.reserve_exact(n);
    let out = image.as_mut_ptr() as *mut u8;
    let rc = if MULTI.load(std::sync::atomic::Ordering::Relaxed) {
        unsafe { fr_render_rgb8_multi(cfg, FR_PRECISION_F64, 0, out, n * 3) }
    } else {
        unsafe { fr_render_rgb8(cfg, out, n * 3) }
    };
    if rc != FR_OK {
        return Err(last_error());
    }
    unsafe { image.set_len(n) }; // every byte was written by the library
    Ok(())
}

/// `get_image`'s `Algo::BarnsleyFern` arm (src/lib.rs:271-319): `threads` is what
/// `rayon::current_num_threads()` returns on this machine (the reference's result is ONE thread's image of
/// `iterations / threads` points), `seed` replaces `SmallRng::from_entropy()` (src/lib.rs:428).
pub fn fern_into<P: Copy>(cfg: &fr_config, threads: u32, seed: u64, image: &mut Vec<P>) -> Result<(), String> {
    assert_eq!(std::mem::size_of::<P>(), 3, "pixel type must be 3 packed bytes");
    let n = cfg.width as usize * cfg.height as usize;
    image.clear();
    image.reserve_exact(n);
    let rc = unsafe { fr_render_fern_rgb8(cfg, threads, seed, 0, image.as_mut_ptr() as *mut u8, n * 3) };
    if rc != FR_OK {
        return Err(last_error());
    }
    unsafe { image.set_len(n) };
    Ok(())
}

/// `calc::get_recursive_pixel(&Config, x, y) -> RGB` (calc/src/lib.rs:199-235) on the device: one pixel per call — the
/// reference's per-pixel API kept for callers that use it; images go through `render_into`.
pub fn get_recursive_pixel(cfg: &fr_config, x: u32, y: u32) -> Result<fr_rgb, String> {
    let mut out = fr_rgb { r: 0, g: 0, b: 0 };
    let rc = unsafe { fr_pixel(cfg, x, y, &mut out) };
    if rc != FR_OK { Err(last_error()) } else { Ok(out) }
}

/// `calc::recursive(iterations, start, c, limit) -> (Imaginary, u32)` (calc/src/lib.rs:245-257): the final position
/// and the escape index (== `iterations` when the cap is exhausted), bit for bit.
pub fn recursive(iterations: u32, start: fr_imaginary, c: fr_imaginary, limit: f64) -> Result<(fr_imaginary, u32), String> {
    let mut pos = fr_imaginary { re: 0.0, im: 0.0 };
    let mut iters = 0u32;
    let rc = unsafe { fr_recursive(iterations, start, c, limit, &mut pos, &mut iters) };
    if rc != FR_OK { Err(last_error()) } else { Ok((pos, iters)) }
}

/// `recursive()` of every pixel of rows `[y0, y1)`: `(z, iters)` with `z[2k], z[2k+1]` the final position and
/// `iters[k]` the escape index of pixel `k = (y - y0) * width + x` — the raw results a GUI keeps to re-colour
/// (`colour_into`) when only exposure / colours / smooth / inside change (src/gui.rs:183-203).
pub fn escape_rows(cfg: &fr_config, y0: u32, y1: u32) -> Result<(Vec<f64>, Vec<u32>), String> {
    let n = cfg.width as usize * (y1.saturating_sub(y0)) as usize;
    let mut z: Vec<f64> = Vec::with_capacity(2 * n);
    let mut iters: Vec<u32> = Vec::with_capacity(n);
    let rc = unsafe { fr_escape_rows(cfg, FR_PRECISION_F64, y0, y1, z.as_mut_ptr(), iters.as_mut_ptr()) };
    if rc != FR_OK {
        return Err(last_error());
    }
    unsafe { z.set_len(2 * n); iters.set_len(n); } // every element was written by the library
    Ok((z, iters))
}

/// Raise the iteration cap of what `escape_rows(cfg_N, y0, y1)` returned, IN PLACE, from `from_iterations` to
/// `cfg.iterations`: only the orbits still running at the old cap are continued, and the arrays then hold what
/// `escape_rows(cfg, y0, y1)` returns, bit for bit (include/fractal_hip.h, `fr_escape_extend_device`) — the GUI's
/// iterations control (src/gui.rs:180) without starting every orbit over.  The arrays must come from the same view at
/// the lower cap; the library cannot check that.
pub fn extend_rows(cfg: &fr_config, y0: u32, y1: u32, from_iterations: u32, z: &mut [f64], iters: &mut [u32]) -> Result<(), String> {
    let n = cfg.width as usize * (y1.saturating_sub(y0)) as usize;
    if z.len() != 2 * n || iters.len() != n {
        return Err(format!("rows [{}, {}) hold {} pixels: z must have {} elements and iters {}", y0, y1, n, 2 * n, n));
    }
    let rc = unsafe { fr_escape_extend(cfg, FR_PRECISION_F64, std::ptr::null(), y0, y1, from_iterations, 2, z.as_mut_ptr(), iters.as_mut_ptr()) };
    if rc != FR_OK { Err(last_error()) } else { Ok(()) }
}

/// The colour map alone (calc/src/lib.rs:214-234 + `color_multiply`) over stored `recursive()` results into a pixel
/// vector: re-colouring without re-iterating.
pub fn colour_into<P: Copy>(cfg: &fr_config, z: &[f64], iters: &[u32], image: &mut Vec<P>) -> Result<(), String> {
    assert_eq!(std::mem::size_of::<P>(), 3, "pixel type must be 3 packed bytes");
    assert_eq!(z.len(), 2 * iters.len());
    let n = iters.len();
    image.clear();
    image.reserve_exact(n);
    let rc = unsafe { fr_colour_rgb8(cfg, z.as_ptr(), iters.as_ptr(), n, image.as_mut_ptr() as *mut u8, n * 3) };
    if rc != FR_OK {
        return Err(last_error());
    }
    unsafe { image.set_len(n) };
    Ok(())
}

/// The whole frame as RGBA8 (r, g, b, 255) into a caller-owned byte buffer of `4 * width * height` bytes: what the GUI
/// builds on the CPU today (`to_rgba8`, src/gui.rs:71-72) produced on the device.  Keep the buffer across frames (and
/// `fr_pin_host_buffer` it once) — see rust/gui.patch.rs.
pub fn render_rgba_into(cfg: &fr_config, frame: &mut [u8]) -> Result<(), String> {
    let need = 4 * cfg.width as usize * cfg.height as usize;
    if frame.len() < need {
        return Err(format!("frame buffer holds {} bytes, the frame needs {}", frame.len(), need));
    }
    let rc = unsafe { fr_render_rows_rgba8(cfg, FR_PRECISION_F64, 0, cfg.height, frame.as_mut_ptr(), frame.len()) };
    if rc != FR_OK { Err(last_error()) } else { Ok(()) }
}

/// `get_image` for a deep zoom (src/gui.rs zooms on scroll without bound): the whole image in double-double arithmetic
/// into a caller-owned pixel vector.  The view centre is `cfg.pos + pos_lo` exactly — `pos_lo` holds the low halves,
/// normalised (`pos.re + pos_lo.re == pos.re` in f64; split a decimal centre with rational arithmetic: hi = nearest
/// f64, lo = nearest f64 to the rest).  `P` must be a 3-byte `#[repr(C)]` pixel.
pub fn get_image_dd<P: Copy>(cfg: &fr_config, pos_lo: fr_imaginary, image: &mut Vec<P>) -> Result<(), String> {
    assert_eq!(std::mem::size_of::<P>(), 3, "pixel type must be 3 packed bytes");
    let n = cfg.width as usize * cfg.height as usize;
    image.clear();
    image.reserve_exact(n);
    let rc = unsafe { fr_render_rows_dd(cfg, &pos_lo, 0, cfg.height, 3, image.as_mut_ptr() as *mut u8, n * 3) };
    if rc != FR_OK {
        return Err(last_error());
    }
    unsafe { image.set_len(n) }; // every byte was written by the library
    Ok(())
}

/// `get_image_dd` in perturbation arithmetic (`FR_PRECISION_PT`): the same deep views at near-f64 cost on long orbits.
/// The view's reference orbit is computed on the host once and kept for the next frames of the same view.
pub fn get_image_pt<P: Copy>(cfg: &fr_config, pos_lo: fr_imaginary, image: &mut Vec<P>) -> Result<(), String> {
    assert_eq!(std::mem::size_of::<P>(), 3, "pixel type must be 3 packed bytes");
    let n = cfg.width as usize * cfg.height as usize;
    image.clear();
    image.reserve_exact(n);
    let rc = unsafe { fr_render_rows_pt(cfg, &pos_lo, 0, cfg.height, 3, image.as_mut_ptr() as *mut u8, n * 3) };
    if rc != FR_OK {
        return Err(last_error());
    }
    unsafe { image.set_len(n) }; // every byte was written by the library
    Ok(())
}

/// `get_image` anti-aliased: the image of `cfg` with `supersample` x `supersample` samples per pixel, box-filtered on the
/// device (include/fractal_hip.h, "supersampled rendering"), into a caller-owned pixel vector.  Only the
/// `width * height` result crosses PCIe.  `pos_lo` is for `FR_PRECISION_DD` / `FR_PRECISION_PT` (see `get_image_dd`),
/// `None` otherwise.  `P` must be a 3-byte `#[repr(C)]` pixel.
pub fn render_ss_into<P: Copy>(cfg: &fr_config, precision: c_int, pos_lo: Option<fr_imaginary>, supersample: u32, image: &mut Vec<P>) -> Result<(), String> {
    assert_eq!(std::mem::size_of::<P>(), 3, "pixel type must be 3 packed bytes");
    let n = cfg.width as usize * cfg.height as usize;
    image.clear();
    image.reserve_exact(n);
    let lo = pos_lo.as_ref().map_or(std::ptr::null(), |p| p as *const fr_imaginary);
    let rc = unsafe { fr_render_rows_ss(cfg, precision, lo, supersample, 0, cfg.height, 3, image.as_mut_ptr() as *mut u8, n * 3, std::ptr::null()) };
    if rc != FR_OK {
        return Err(last_error());
    }
    unsafe { image.set_len(n) }; // every byte was written by the library
    Ok(())
}

/// The loaded library must speak the ABI these declarations describe (include/fractal_hip.h: FR_ABI_VERSION).
pub fn check_abi() -> Result<(), String> {
    let v = unsafe { fr_abi_version() };
    if v == FR_ABI_VERSION { Ok(()) } else { Err(format!("libfractal_hip speaks ABI {}, this crate {}", v, FR_ABI_VERSION)) }
}
