// nsk_seg_table.h -- the kernel-argument tables of the segment launches, as plain data: the kernels
// (nsk_kernels_gibbs.h, nsk_kernels_learn.h) read them, the host-only planner (nsk_seg_plan.h) fills them.  No HIP type.
// Layout and field order are the kernels' argument layout.
#pragma once

#include <stdint.h>

namespace nsk {

// Homogeneous segments: runs of consecutive uniform tiles with one program, slot count, kind and
// evidence flag (the shape-class layout of nsk_compile.cpp makes whole classes such runs).  Up to
// NSK_SEG_MAX segments of one (kind, chunk count) share a launch; everything the descriptor-driven
// kernel fetches per tile comes from the kernel-argument table here, and the body is straight
// line: ids, 16-byte member loads, byte gathers, compares, draw, store.
#define NSK_SEG_MAX 8
#define NSK_NO_STREAM 0xFFFFFFFFu          // SegEntry.aff_off of a segment without implicit adjacency
struct SegEntry {                         // 48 bytes: two scalar loads per tile (pair)
    int tile_start;                       // first tile of the segment in this launch's numbering
    int pos0;                             // position of the segment's first lane
    uint32_t adj_off;                     // stream offset (16-byte units) of its first tile
    uint32_t prog;                        // slot program
    uint32_t zoff;                        // draw-table launches: first entry of the program's table
    uint32_t zmask_ev;                    // (1 << member slots) - 1 | (uint8) common isEvidence << 8 | quad generator scheme << 16
    uint32_t ntiles_lead;                 // table launches: tiles of the segment | lead << 30 (dead virtual
                                          //   tiles in front: the segment does not start a quad)
    uint32_t aff_off;                     // first entry of the segment's tiles in seg_aff, NSK_NO_STREAM: none
    uint32_t push_off;                    // fused boundary exchange (TabP2P): first row of the segment's tiles in the
                                          //   push map, NSK_NO_STREAM: no tile of the segment touches the boundary
    uint32_t wide_off;                    // table launches: first dword of the quad descriptors (seg_wide) from the quad of
                                          //   pos0 on, NSK_NO_STREAM: none (int32 values, NSK_NO_WIDE)
    uint32_t pad_[2];
};
struct SegTable {
    int n, ntiles;                        // segments, tiles of the launch; e[i].tile_start = ntiles for i >= n
    int wide, pad_;                       // table launches: some segment has quad descriptors (SegEntry.wide_off)
    SegEntry e[NSK_SEG_MAX];
};

#define NSK_TABW_REST_MAX 64        // quads of a wide launch that are not wide ones and get a workgroup of their own (TabwCold.rest)

}  // namespace nsk
