// lfx_verdict.h — host only, no HIP: what the host makes of a container and of a decode's verdict — the trailer's length and
// checksum kind, status and message text, the trailer compare.  The decode's host sources and the stream decoder's state
// machine (lfx_stream_dec.h, built by a plain host compiler) include it; nothing a kernel reads is here.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "../../include/lfx.h"
#include "lfx_blk.h"

namespace lfx {

// the checksum a container's trailer holds, as launch_checksum's mode (raw DEFLATE: none), and the trailer's bytes
// (gzip: CRC-32 + ISIZE, zlib: Adler-32)
inline int ck_mode_of(int format) { return format == LFX_GZIP ? 1 : format == LFX_ZLIB ? 2 : 0; }
inline uint32_t trailer_len(int format) { return format == LFX_GZIP ? 8 : format == LFX_ZLIB ? 4 : 0; }

inline int map_status(uint32_t st) {
    return st == 0 ? LFX_OK : st == 1 ? LFX_E_INVALID_DATA : st == 2 ? LFX_E_UNEXPECTED_EOF : LFX_E_NOSPACE;
}
// messages: prefixes match the reference texts quoted in SURVEY.md §4
inline std::string format_error(uint32_t err, uint32_t a0, uint32_t a1) {
    char m[200];
    switch (err) {
        case ERR_EOF: return "failed to fill whole buffer";
        case ERR_HUFF: return "Invalid huffman coded stream";
        case ERR_CONFLICT: snprintf(m, sizeof m, "Bit region conflict: symbol=%u", a0); return m;
        case ERR_HDIST: snprintf(m, sizeof m, "The value of HDIST is too big: max=30, actual=%u", a0); return m;
        case ERR_NO_PREV: return "No preceding value";
        case ERR_DIST_LIST:
            snprintf(m, sizeof m, "The length of `distance_code_bitwidthes` is too large: actual=%u, expected=%u", a0, a1);
            return m;
        case ERR_286: snprintf(m, sizeof m, "The value %u must not occur in compressed data", a0); return m;
        case ERR_BACKREF: snprintf(m, sizeof m, "Too long backword reference: buffer.len=%u, distance=%u", a0, a1); return m;
        case ERR_BTYPE3: return "btype 0x11 of DEFLATE is reserved(error) value";
        case ERR_LEN_NLEN: snprintf(m, sizeof m, "LEN=%u is not the one's complement of NLEN=%u", a0, a1); return m;
        case ERR_STORED_SHORT: snprintf(m, sizeof m, "The reader has incorrect length: expected %u, read %u", a0, a1); return m;
        case ERR_NOSPACE: return "output capacity too small";
        case ERR_ZLIB_CHECK:
            snprintf(m, sizeof m, "Inconsistent ZLIB check bits: `CMF(%u) * 256 + FLG(%u)` must be a multiple of 31", a0, a1);
            return m;
        case ERR_METHOD: snprintf(m, sizeof m, "Compression methods other than DEFLATE(8) are unsupported: method=%u", a0); return m;
        case ERR_CINFO: snprintf(m, sizeof m, "CINFO above 7 are not allowed: value=%u", a0); return m;
        case ERR_FDICT: snprintf(m, sizeof m, "Preset dictionaries are not supported: dictionary_id=0x%X", a0); return m;
        case ERR_GZIP_ID: return "Unexpected GZIP ID";
        case ERR_HCRC: snprintf(m, sizeof m, "CRC16 of GZIP header mismatched: value=%u, expected=%u", a0, a1); return m;
        case ERR_CRC32: snprintf(m, sizeof m, "CRC32 mismatched: value=%u, expected=%u", a0, a1); return m;
        case ERR_ADLER32: snprintf(m, sizeof m, "Adler32 checksum mismatched: value=%u, expected=%u", a0, a1); return m;
        case ERR_DICT_MISMATCH: snprintf(m, sizeof m, "Dictionary mismatch: dictionary_id=0x%X, supplied=0x%X", a0, a1); return m;
        default: return "";
    }
}

// the checksum of a member's output against its trailer t[0, trailer_len(format)): gzip holds the CRC-32 little-endian
// (gzip.rs:1035-1040; ISIZE is read but never verified), zlib the Adler-32 big-endian (zlib.rs:396-401).
// → LFX_OK, or LFX_E_INVALID_DATA with the reference's text in msg
inline int check_trailer(int format, const uint8_t *t, uint32_t crc32, uint32_t adler32, std::string &msg) {
    if (format == LFX_GZIP) {
        const uint32_t crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        if (crc != crc32) { msg = format_error(ERR_CRC32, crc32, crc); return LFX_E_INVALID_DATA; }
    } else if (format == LFX_ZLIB) {
        const uint32_t ad = (uint32_t)t[0] << 24 | (uint32_t)t[1] << 16 | (uint32_t)t[2] << 8 | t[3];
        if (ad != adler32) { msg = format_error(ERR_ADLER32, adler32, ad); return LFX_E_INVALID_DATA; }
    }
    return LFX_OK;
}

}  // namespace lfx
