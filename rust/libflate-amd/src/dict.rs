//! Preset dictionaries (include/lfx.h): what `deflateSetDictionary` is given.  A `Dictionary` is made
//! once per context and handed to `zlib::Encoder::with_dictionary` / `deflate::Encoder::with_dictionary`, which keep it alive.
//! The raw bindings of the dictionary calls live here, next to their only user (tests/test_stream_dict_abi.py holds the
//! constructor's line against the header).
#![allow(non_camel_case_types)]
use std::io;
use std::os::raw::{c_int, c_void};
use std::sync::Arc;

use crate::ffi::{lfx_ctx, lfx_encode_opts, lfx_encoder, lfx_flush_cb, lfx_write_cb};
use crate::{default_context, io_error, Context};

pub enum lfx_dict {}

extern "C" {
    pub fn lfx_dict_new(c: *mut lfx_ctx, bytes: *const c_void, len: u64, on_device: c_int, status: *mut c_int) -> *mut lfx_dict;
    pub fn lfx_dict_new_chain(c: *mut lfx_ctx, bytes: *const c_void, len: u64, on_device: c_int, status: *mut c_int) -> *mut lfx_dict;
    pub fn lfx_dict_id(d: *const lfx_dict) -> u32;
    pub fn lfx_dict_free(d: *mut lfx_dict);
    pub fn lfx_encoder_new_dict(c: *mut lfx_ctx, format: c_int, o: *const lfx_encode_opts, dict: *const lfx_dict, w: lfx_write_cb, f: Option<lfx_flush_cb>, user: *mut c_void, status: *mut c_int) -> *mut lfx_encoder;
}

/// A preset dictionary of the default context.  Its last 32 KiB are the usable history; `id()` is the Adler-32 of all bytes
/// (RFC 1950's DICTID).
pub struct Dictionary {
    pub(crate) h: *mut lfx_dict,
    pub(crate) ctx: Arc<Context>,
}
unsafe impl Send for Dictionary {}
unsafe impl Sync for Dictionary {}
impl Dictionary {
    /// for the default parse (`lfx_dict_new`)
    pub fn new(bytes: &[u8]) -> io::Result<Arc<Dictionary>> { Self::make(bytes, false) }
    /// with the hash chain of its own tail: what `ChainLz77Encoder`, `LazyLz77Encoder` and `LevelLz77Encoder` need
    /// (`lfx_dict_new_chain`); for every other parse it is the same dictionary
    pub fn with_chain(bytes: &[u8]) -> io::Result<Arc<Dictionary>> { Self::make(bytes, true) }
    fn make(bytes: &[u8], chain: bool) -> io::Result<Arc<Dictionary>> {
        let ctx = default_context()?;
        let mut st: c_int = 0;
        let h = unsafe {
            if chain { lfx_dict_new_chain(ctx.0, bytes.as_ptr() as *const c_void, bytes.len() as u64, 0, &mut st) }
            else { lfx_dict_new(ctx.0, bytes.as_ptr() as *const c_void, bytes.len() as u64, 0, &mut st) }
        };
        if h.is_null() {
            return Err(io_error(st, format!("dictionary construction failed: {}", ctx.last_error())));
        }
        Ok(Arc::new(Dictionary { h, ctx }))
    }
    pub fn id(&self) -> u32 { unsafe { lfx_dict_id(self.h) } }
}
impl Drop for Dictionary {
    fn drop(&mut self) { unsafe { lfx_dict_free(self.h) } }
}
