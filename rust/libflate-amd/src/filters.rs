//! The byte-shuffle filter for numeric records (include/lfx.h "the byte-shuffle filter"): HDF5's
//! H5Z_FILTER_SHUFFLE, numcodecs' Shuffle.  Declarations only — the calls take raw device or host pointers and are driven from
//! Python and from C; this crate adds no safe wrapper yet.  (ffi.rs holds the externs tests/c/shim_abi.c drives.)
use std::os::raw::{c_int, c_void};

use crate::ffi::lfx_ctx;

pub const LFX_SHUFFLE: c_int = 0;
pub const LFX_UNSHUFFLE: c_int = 1;

extern "C" {
    pub fn lfx_shuffle_device(c: *mut lfx_ctx, dir: c_int, elem_size: u32, d_in: *const c_void, n: u64, d_out: *mut c_void) -> c_int;
    pub fn lfx_shuffle_batch_device(c: *mut lfx_ctx, dir: c_int, elem_size: u32, count: u32, d_in: *const c_void, in_off: *const u64, len: *const u64, d_table: *const c_void, d_out: *mut c_void, out_off: *const u64) -> c_int;
    pub fn lfx_shuffle_host(c: *mut lfx_ctx, dir: c_int, elem_size: u32, input: *const c_void, n: u64, out: *mut c_void) -> c_int;
}
