//! astroz_hip.zig -- the FFI shim a maintainer of ATTron/astroz adds as src/hip.zig: every entry point of
//! include/astroz_hip.h as a Zig `extern "c"` declaration, plus the AZ_ERR_* -> Zig error mapping.
//! Link with `-lastroz_hip`.  Zig is not installed in this repository's build image, so this file is not compiled
//! here; tests/test_host_cpu.py::test_zig_shim_matches_header checks it against the header (every exported name,
//! its parameter count), and the same call sequences are compiled and run from C (tests/c_client/client.c).
//! Reference interfaces replaced: src/Constellation.zig L245-308, L541-679; src/c_api/root.zig L13-81;
//! src/dispatch.zig L18-54.

/// include/astroz_hip.h AZ_ERR_* (= src/c_api/error.zig L3-19) -> the error sets the reference's callers expect
/// (Sgp4.Error / Sdp4.Error members where they exist, src/Sgp4.zig L26-31).
pub const HipError = error{
    BadTleLength,
    BadChecksum,
    DeepSpaceNotSupported,
    InvalidEccentricity,
    SatelliteDecayed,
    ValueError,
    OutOfMemory,
    NullPointer,
    NotInitialized,
    /// AZ_ERR_HIP: no device, a failed launch or copy (text: azh_last_error())
    DeviceFailure,
    Unknown,
};

pub fn check(rc: i32) HipError!void {
    return switch (rc) {
        0 => {},
        -1 => HipError.BadTleLength,
        -2 => HipError.BadChecksum,
        -10 => HipError.DeepSpaceNotSupported,
        -11 => HipError.InvalidEccentricity,
        -12 => HipError.SatelliteDecayed,
        -20 => HipError.ValueError,
        -100 => HipError.OutOfMemory,
        -101 => HipError.NullPointer,
        -102 => HipError.NotInitialized,
        -200 => HipError.DeviceFailure,
        else => HipError.Unknown,
    };
}

pub const Handle = opaque {};

pub const Err = enum(i32) {
    ok = 0,
    bad_tle_length = -1,
    bad_checksum = -2,
    deep_space_not_supported = -10,
    invalid_eccentricity = -11,
    satellite_decayed = -12,
    value_error = -20,
    alloc_failed = -100,
    null_pointer = -101,
    not_initialized = -102,
    hip = -200,
    unknown = -999,
};

pub extern "c" fn azh_device_count() c_int;
pub extern "c" fn azh_last_error() [*:0]const u8;
pub extern "c" fn azh_parse_tle_lines(line1: [*:0]const u8, line2: [*:0]const u8, out16: [*]f64) i32;
pub extern "c" fn azh_constellation_from_tle_text(text: [*]const u8, len: usize, grav: i32, device: i32, out: *?*Handle) i32;
pub extern "c" fn azh_constellation_from_tle_lines(line1: [*]const [*:0]const u8, line2: [*]const [*:0]const u8, n: usize, grav: i32, device: i32, out: *?*Handle) i32;
pub extern "c" fn azh_constellation_from_elements(n: usize, epoch_jd: [*]const f64, mm_revday: [*]const f64, ecc: [*]const f64, incl_deg: [*]const f64, raan_deg: [*]const f64, argp_deg: [*]const f64, ma_deg: [*]const f64, bstar: [*]const f64, grav: i32, device: i32, out: *?*Handle) i32;
pub extern "c" fn azh_constellation_free(h: ?*Handle) void;
pub extern "c" fn azh_num_satellites(h: ?*const Handle) usize;
pub extern "c" fn azh_num_sgp4(h: ?*const Handle) usize;
pub extern "c" fn azh_num_sdp4(h: ?*const Handle) usize;
pub extern "c" fn azh_get_epochs(h: ?*const Handle, out: [*]f64) i32;
pub extern "c" fn azh_get_status(h: ?*const Handle, err: ?[*]u8, is_deep: ?[*]u8, irez: ?[*]u8) i32;
pub extern "c" fn azh_get_field(h: ?*const Handle, name: [*:0]const u8, out: [*]f64) i32;
pub extern "c" fn azh_propagate_host(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64, pos: [*]f64, vel: ?[*]f64, output_mode: i32, reference_jd: f64, sat_mask: ?[*]const u8, layout: i32, out_stride_sats: usize, err: ?[*]u8) i32;
pub extern "c" fn azh_propagate_device(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64, d_pos: [*]f64, d_vel: ?[*]f64, output_mode: i32, reference_jd: f64, sat_mask: ?[*]const u8, layout: i32, out_stride_sats: usize, d_err: ?[*]u8, stream: ?*anyopaque) i32;
pub extern "c" fn azh_propagate_device_cached(h: ?*Handle, d_pos: [*]f64, d_vel: ?[*]f64, layout: i32, out_stride_sats: usize, d_err: ?[*]u8, stream: ?*anyopaque) i32;
pub extern "c" fn azh_propagate_jd_host(h: ?*Handle, jd: [*]const f64, fr: [*]const f64, n_times: usize, pos: [*]f64, vel: ?[*]f64, output_mode: i32, layout: i32, err: ?[*]u8) i32;
pub extern "c" fn azh_propagate_one_host(h: ?*Handle, sat_index: usize, tsince_min: [*]const f64, n: usize, pos: [*]f64, vel: ?[*]f64, err: ?[*]u8) i32;
pub extern "c" fn azh_synchronize(h: ?*Handle) i32;
pub extern "c" fn azh_set_time_tile(h: ?*Handle, sgp4_tile: u32, sdp4_tile: u32) i32;
pub extern "c" fn azh_set_timing(h: ?*Handle, enabled: i32) i32;
pub extern "c" fn azh_last_kernel_ms(h: ?*Handle) f64;

// fp32 outputs (config 5)
pub extern "c" fn azh_propagate_device_f32(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    d_pos: [*]f32, d_vel: ?[*]f32, output_mode: i32, reference_jd: f64, sat_mask: ?[*]const u8, layout: i32,
    out_stride_sats: usize, d_err: ?[*]u8, stream: ?*anyopaque) i32;
pub extern "c" fn azh_propagate_device_cached_f32(h: ?*Handle, d_pos: [*]f32, d_vel: ?[*]f32, layout: i32,
    out_stride_sats: usize, d_err: ?[*]u8, stream: ?*anyopaque) i32;

// conjunction screening: Constellation.screenConstellation (src/Constellation.zig L683-756) and
// coarseScreen (bindings/python/src/conjunction.zig L11-150)
pub extern "c" fn azh_screen_target_host(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    target_index: usize, threshold_km: f64, reference_jd: f64, min_dist_km: [*]f64, min_t_index: [*]u32) i32;
pub extern "c" fn azh_screen_target_device(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    target_index: usize, threshold_km: f64, reference_jd: f64, d_min_dist_km: [*]f64, d_min_t_index: [*]u32, stream: ?*anyopaque) i32;
pub extern "c" fn azh_screen_track_device(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    d_track: [*]const f64, exclude_index: usize, threshold_km: f64, d_min_dist_km: [*]f64, d_min_t_index: [*]u32, stream: ?*anyopaque) i32; // the same against an external track (another shard's satellite)
pub extern "c" fn azh_coarse_screen_device(d_pos: [*]const f64, n_sats: usize, n_times: usize, layout: i32, stride_sats: usize,
    threshold_km: f64, valid_mask: ?[*]const u8, out_pairs: [*]u32, out_t_index: [*]u32, max_results: usize, n_found: *usize,
    stream: ?*anyopaque) i32;
pub extern "c" fn azh_coarse_screen_host(pos: [*]const f64, n_sats: usize, n_times: usize, layout: i32, stride_sats: usize,
    threshold_km: f64, valid_mask: ?[*]const u8, out_pairs: [*]u32, out_t_index: [*]u32, max_results: usize, n_found: *usize,
    device: i32) i32;
pub extern "c" fn azh_screen_all_host(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    threshold_km: f64, out_pairs: [*]u32, out_t_index: [*]u32, max_results: usize, n_found: *usize) i32;

// ---- round 2 ----
// text front ends (Tle.MultiIterator / parseOmm / parseOmmArray, src/Tle.zig L103-238)
pub extern "c" fn azh_parse_tle_text(text: [*]const u8, len: usize, out16: [*]f64, max_records: usize, n_found: *usize) i32;
pub extern "c" fn azh_parse_omm_json(text: [*]const u8, len: usize, out16: [*]f64, max_records: usize, n_found: *usize) i32;
pub extern "c" fn azh_set_parse_threads(n: i32) void;
pub extern "c" fn azh_constellation_from_omm_json(text: [*]const u8, len: usize, grav: i32, device: i32, out: *?*Handle) i32;
pub extern "c" fn azh_constellation_subset(h: ?*const Handle, indices: [*]const u32, n: usize, device: i32, out: *?*Handle) i32;

// row windows (chunked multi-GPU pipelines), arithmetic / path switches, device-pointer one-satellite call
pub extern "c" fn azh_propagate_device_window(h: ?*Handle, row_lo: usize, row_hi: usize, d_pos: [*]f64, d_vel: ?[*]f64, layout: i32,
    out_stride_sats: usize, d_err: ?[*]u8, stream: ?*anyopaque) i32;
pub extern "c" fn azh_set_f32_mode(h: ?*Handle, mode: i32) i32; // 0 mixed precision (default), 1 packed fp32, 2 fp64 rounded at the store
pub extern "c" fn azh_set_f32_arithmetic(h: ?*Handle, enabled: i32) i32; // boolean: 0 = fp64 rounded at the store, else packed fp32
pub extern "c" fn azh_set_fast_path(h: ?*Handle, enabled: i32) i32;
pub extern "c" fn azh_set_tile_kernel(h: ?*Handle, enabled: i32) i32;
pub extern "c" fn azh_set_graphs(h: ?*Handle, enabled: i32) i32; // hipGraph replay of repeated cached-input launch sets (default off; pays for multi-window pipelines)
pub extern "c" fn azh_set_host_points(n: usize) void; // one-satellite calls of at most n points run the library's step on the calling thread (default 128; deep-space members: half)
pub extern "c" fn azh_get_host_points() usize;
pub extern "c" fn azh_set_host_copy_threads(n: i32) void; // host threads behind the pinned staging of host-returning copies (-1 auto, 0 = direct pageable copies)
// result arrays the DMA engines write directly (pinned, pooled inside the library): a Zig host allocates `positions` / `velocities`
// here instead of from its allocator, and azh_propagate_host lands in them at the link rate (no staging hop)
pub extern "c" fn azh_host_alloc(bytes: usize, out: *?*anyopaque) i32;
pub extern "c" fn azh_host_free(p: ?*anyopaque) void;
pub extern "c" fn azh_host_pool_stats(live_bytes: ?*usize, free_bytes: ?*usize) void;
pub extern "c" fn azh_host_pool_trim() void;
pub extern "c" fn azh_last_path(h: ?*const Handle) u32; // AZH_PATH_* bits: which kernel families the last call launched
pub extern "c" fn azh_last_one_stats(h: ?*Handle, n_segments: ?*u32, n_handed_over: ?*u32) i32; // last one-satellite call: fast segments / handed over
pub extern "c" fn azh_last_window_tiers(h: ?*Handle, counts: *[4]u32) i32; // windows of the last plan per loop body: general, eps, eccentric, rejected
pub extern "c" fn azh_last_window_ecc_tiers(h: ?*Handle, counts: *[3]u32) i32; // its eccentric windows per loop body: E1, E2, general
pub extern "c" fn azh_propagate_one_device(h: ?*Handle, sat_index: usize, d_tsince_min: [*]const f64, n: usize, d_pos: [*]f64,
    d_vel: ?[*]f64, d_err: ?[*]u8, stream: ?*anyopaque) i32;
pub extern "c" fn azh_selftest_math(x: [*]const f64, n: usize, out6n: [*]f64, device: i32) i32;
pub extern "c" fn azh_selftest_host_step(el: [*]const f64, n_pad: usize, sat: usize, flags: u32, grav: i32, tsince_min: [*]const f64, n: usize,
    out6n: [*]f64, err: ?[*]u8) i32; // the host route's step on a caller-supplied element table (no device needed; KAT)
pub extern "c" fn azh_selftest_coords(op: i32, in: *const [4]f64, out: *[5]f64) i32; // part (A)'s closed forms through the kernels' frame code (KAT)

// src/c_api/coords.zig
pub extern "c" fn coords_julian_to_gmst(jd: f64) f64;
pub extern "c" fn coords_eci_to_ecef(eci: *const [3]f64, gmst: f64, ecef: *[3]f64) void;
pub extern "c" fn coords_ecef_to_geodetic(ecef: *const [3]f64, lla: *[3]f64) void;
pub extern "c" fn azh_coords_topocentric(r_teme: *const [3]f64, v_teme: ?*const [3]f64, gmst: f64, observer_lla: *const [3]f64,
    aer: *[3]f64, aer_rate: ?*[3]f64) void; // host twin of the AZ_OUT_TOPOCENTRIC epilogue

// ground-station look angles (output_mode 3 = AZ_OUT_TOPOCENTRIC) and pass prediction
pub const OUT_TOPOCENTRIC: i32 = 3;
pub const Pass = extern struct {
    t_rise_min: f64,
    t_culm_min: f64,
    t_set_min: f64,
    max_elevation_rad: f64,
    rise_azimuth_rad: f64,
    set_azimuth_rad: f64,
    flags: u32, // PASS_*
    grid_rise: u32,
    grid_culm: u32,
    grid_set: u32,
};
pub const PASS_UP_AT_START: u32 = 1;
pub const PASS_UP_AT_END: u32 = 2;
pub const PASS_CUT_BY_ERROR: u32 = 4;
pub extern "c" fn azh_set_observer(h: ?*Handle, lat_deg: f64, lon_deg: f64, alt_km: f64) i32;
pub extern "c" fn azh_find_passes_host(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    reference_jd: f64, min_elevation_deg: f64, out: [*]Pass, max_passes: usize, n_passes: [*]u32) i32;
pub extern "c" fn azh_find_passes_device(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    reference_jd: f64, min_elevation_deg: f64, d_out: [*]Pass, max_passes: usize, d_n_passes: [*]u32, stream: ?*anyopaque) i32;
pub extern "c" fn azh_find_passes_stations_host(h: ?*Handle, times_min: [*]const f64, n_times: usize,
    epoch_offsets_min: ?[*]const f64, reference_jd: f64, stations_lla: [*]const [3]f64, min_elevation_deg: [*]const f64,
    n_stations: usize, out: [*]Pass, max_passes: usize, n_passes: [*]u32) i32;
pub extern "c" fn azh_find_passes_stations_device(h: ?*Handle, times_min: [*]const f64, n_times: usize,
    epoch_offsets_min: ?[*]const f64, reference_jd: f64, stations_lla: [*]const [3]f64, min_elevation_deg: [*]const f64,
    n_stations: usize, d_out: [*]Pass, max_passes: usize, d_n_passes: [*]u32, stream: ?*anyopaque) i32;

// ground coverage: satellites in view per (ground point, grid time) and the statistics of every point's series
pub const Coverage = extern struct {
    mean_in_view: f64,
    max_gap_min: f64,
    n_covered: u32,
    min_in_view: u32,
    max_in_view: u32,
    n_gaps: u32,
    grid_gap_start: u32,
    grid_gap_end: u32,
    flags: u32,
    reserved: u32,
};
pub const COVERAGE_GAP_AT_START: u32 = 1;
pub const COVERAGE_GAP_AT_END: u32 = 2;
pub extern "c" fn azh_coverage_host(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    reference_jd: f64, points_lla: [*]const [3]f64, min_elevation_deg: [*]const f64, n_points: usize, min_satellites: u32,
    stats: [*]Coverage, counts_or_null: ?[*]u32) i32;
pub extern "c" fn azh_coverage_device(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    reference_jd: f64, points_lla: [*]const [3]f64, min_elevation_deg: [*]const f64, n_points: usize, min_satellites: u32,
    d_stats: [*]Coverage, d_counts_or_null: ?[*]u32, stream: ?*anyopaque) i32;

// the Sun, the Earth's shadow and eclipse intervals
pub extern "c" fn azh_sun_position_teme(jd: f64, sun_km: *[3]f64) void; // Almanac low-precision series (Vallado, "Sun"), km
pub extern "c" fn azh_selftest_sun(jd: [*]const f64, n: usize, out3n: [*]f64, device: i32) i32; // the device twin (KAT)
pub extern "c" fn azh_shadow_state(r_teme: *const [3]f64, sun_km: *const [3]f64, f_umbra: ?*f64, f_penumbra: ?*f64) i32; // 0 sunlit, 1 penumbra, 2 umbra
pub const Eclipse = extern struct {
    t_entry_min: f64,
    t_exit_min: f64,
    flags: u32, // ECLIPSE_*
    grid_entry: u32,
    grid_exit: u32,
    reserved: u32,
};
pub const ECLIPSE_IN_AT_START: u32 = 1;
pub const ECLIPSE_IN_AT_END: u32 = 2;
pub const ECLIPSE_CUT_BY_ERROR: u32 = 4;
pub const SHADOW_UMBRA: i32 = 0;
pub const SHADOW_PENUMBRA: i32 = 1;
pub extern "c" fn azh_find_eclipses_host(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    reference_jd: f64, kind: i32, out: ?[*]Eclipse, max_eclipses: usize, n_eclipses: [*]u32, state_or_null: ?[*]u8) i32;
pub extern "c" fn azh_find_eclipses_device(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    reference_jd: f64, kind: i32, d_out: ?[*]Eclipse, max_eclipses: usize, d_n_eclipses: [*]u32, d_state_or_null: ?[*]u8,
    stream: ?*anyopaque) i32;

// line of sight past a spherical Earth and access windows between a target and every member
pub extern "c" fn azh_line_of_sight(r1: *const [3]f64, r2: *const [3]f64, grazing_alt_km: f64, clearance_km: ?*f64, range_km: ?*f64) i32; // 1 clear, 0 blocked
pub const Access = extern struct {
    t_start_min: f64,
    t_end_min: f64,
    min_range_km: f64,
    flags: u32, // ACCESS_*
    grid_start: u32,
    grid_end: u32,
    grid_min_range: u32,
};
pub const ACCESS_OPEN_AT_START: u32 = 1;
pub const ACCESS_OPEN_AT_END: u32 = 2;
pub const ACCESS_CUT_BY_ERROR: u32 = 4;
pub const NO_TARGET: usize = ~@as(usize, 0); // exclude_index of azh_find_access_track_device: leave no member out
pub extern "c" fn azh_find_access_host(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    target_index: usize, grazing_alt_km: f64, max_range_km: f64, out: ?[*]Access, max_windows: usize, n_windows: [*]u32,
    state_or_null: ?[*]u8) i32;
pub extern "c" fn azh_find_access_device(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    target_index: usize, grazing_alt_km: f64, max_range_km: f64, d_out: ?[*]Access, max_windows: usize, d_n_windows: [*]u32,
    d_state_or_null: ?[*]u8, stream: ?*anyopaque) i32;
pub extern "c" fn azh_find_access_track_device(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    d_track_pos: [*]const f64, d_track_vel: [*]const f64, exclude_index: usize, grazing_alt_km: f64, max_range_km: f64,
    d_out: ?[*]Access, max_windows: usize, d_n_windows: [*]u32, d_state_or_null: ?[*]u8, stream: ?*anyopaque) i32;

// refined close approaches between a fleet of targets and every member
pub extern "c" fn azh_closest_approach(d0: *const [3]f64, w0: *const [3]f64, d1: *const [3]f64, w1: *const [3]f64, dt_min: f64,
    sigma: ?*f64, miss_km: ?*f64, rel_speed_km_s: ?*f64) i32; // 1 bracket (outputs written), 0 none
pub const Conjunction = extern struct {
    t_tca_min: f64,
    miss_km: f64,
    rel_speed_km_s: f64,
    target: u32, // slot in targets[]
    sat: u32, // catalog row
    grid_index: u32, // left end of the bracket
    reserved: u32,
};
pub extern "c" fn azh_find_conjunctions_host(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    targets: [*]const usize, n_targets: usize, threshold_km: f64, out: ?[*]Conjunction, max_events: usize, n_events: *u32) i32;
pub extern "c" fn azh_find_conjunctions_device(h: ?*Handle, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    targets: [*]const usize, n_targets: usize, threshold_km: f64, d_out: ?[*]Conjunction, max_events: usize, d_n_events: *u32,
    stream: ?*anyopaque) i32;

// one process, several devices: replaces the std.Thread fan-out of Constellation.propagateConstellation
// (src/Constellation.zig L557-603)
pub const Group = opaque {};
pub extern "c" fn azh_group_create_from_tle_text(text: [*]const u8, len: usize, grav: i32, devices: [*]const i32, n_devices: i32,
    n_chunks: i32, out: *?*Group) i32;
pub extern "c" fn azh_group_create_from_omm_json(text: [*]const u8, len: usize, grav: i32, devices: [*]const i32, n_devices: i32,
    n_chunks: i32, out: *?*Group) i32;
pub extern "c" fn azh_group_free(g: ?*Group) void;
pub extern "c" fn azh_group_num_satellites(g: ?*const Group) usize;
pub extern "c" fn azh_group_num_devices(g: ?*const Group) i32;
pub extern "c" fn azh_group_padded_rows(g: ?*const Group) usize;
pub extern "c" fn azh_group_get_epochs(g: ?*const Group, out: [*]f64) i32;
pub extern "c" fn azh_group_propagate_host(g: ?*Group, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    n_offsets: usize, pos: [*]f64, vel: ?[*]f64, output_mode: i32, reference_jd: f64, err: ?[*]u8) i32;
pub extern "c" fn azh_group_propagate_allgather(g: ?*Group, times_min: [*]const f64, n_times: usize,
    epoch_offsets_min: ?[*]const f64, n_offsets: usize, d_pos: [*]const [*]f64, d_vel: ?[*]const [*]f64) i32;
// the fused single-target screen over a group (Constellation.screenConstellation, src/Constellation.zig L683-756): every device
// screens its own rows against the target's track, no collective
pub extern "c" fn azh_group_screen_target_host(g: ?*Group, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    n_offsets: usize, target_index: usize, threshold_km: f64, reference_jd: f64, min_dist_km: [*]f64, min_t_index: [*]u32) i32;
pub extern "c" fn azh_group_screen_target_device(g: ?*Group, times_min: [*]const f64, n_times: usize, epoch_offsets_min: ?[*]const f64,
    n_offsets: usize, target_index: usize, threshold_km: f64, reference_jd: f64, d_min_dist_km: [*]const [*]f64, d_min_t_index: [*]const [*]u32) i32;
pub extern "c" fn azh_group_shard_size(g: ?*const Group, device_slot: i32) usize;
pub extern "c" fn azh_group_shard_rows(g: ?*const Group, device_slot: i32, out_rows: [*]u32) i32;
pub extern "c" fn azh_group_synchronize(g: ?*Group) i32;
