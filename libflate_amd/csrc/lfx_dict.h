// lfx_dict.h — a preset dictionary (C ABI: lfx_dict_*) as the decode paths see it.  Internal.
#pragma once
#include <stdint.h>

#include <vector>

#include "lfx_common.h"

namespace lfx { struct Ctx; }

// The usable history is the dictionary's last min(len, 32768) bytes.  On the device they END a 32 KiB window (d_win, zeros in
// front of them): the shape of the marker path's init_win, and d_win + 32768 is the dict_end of the dictionary kernels.  The
// same bytes on the host seed a stream decoder's first window.  id = Adler-32 of ALL bytes (RFC 1950's DICTID).
struct lfx_dict {
    lfx::Ctx *c = nullptr;
    uint32_t id = 1;
    uint32_t usable = 0;
    uint8_t *d_win = nullptr;
    std::vector<uint8_t> tail;
    const uint8_t *d_end() const { return d_win + lfx::MAX_WINDOW; }
};
