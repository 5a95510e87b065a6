// Bookkeeping of the fused GroupNorm epilogues' statistics exchange (trunk_f16x3_common.h: gnx_publish / gnx_collect), with no HIP in it: what a
// granule is, which record a tile publishes and which records it reads, how many records a layer needs and how the pass epoch
// moves.  The kernels and the workspace layout call these functions; tests/gn_exchange_main.cpp drives the same code on the CPU
// under the host sanitizers.
//
// A tile of a fused conv whose image is spread over several row tiles publishes ONE record: kGnxGranules granules of 8 bytes, each
// {fp32 partial sum, tag}, stored by one wave in one 8-byte-per-lane store instruction.  The tag is the epoch of the pass that
// wrote the granule, so a reader tells a value of this pass from whatever an earlier pass left there without anybody zeroing
// records between passes, and learns "written" and the value from the same load.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SERL_GNX_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define SERL_GNX_HD inline
#endif

namespace serl {

constexpr int kGnxGranules = 32;                     // per record: 4 waves x (up to) 4 sixteen-channel segments x {sum, sumsq}
constexpr int kGnxRecordBytes = kGnxGranules * 8;

SERL_GNX_HD uint64_t gnx_pack(uint32_t value_bits, uint32_t tag) { return ((uint64_t)tag << 32) | value_bits; }
SERL_GNX_HD uint32_t gnx_tag(uint64_t granule) { return (uint32_t)(granule >> 32); }
SERL_GNX_HD uint32_t gnx_value(uint64_t granule) { return (uint32_t)granule; }

// EPOCH RULE.  A workspace counts its passes; the count is the tag of every granule of the pass and is never 0.  Records are not
// zeroed between passes.  They ARE zeroed (tag 0 = no pass) before the workspace's first pass, whose memory holds anything, and
// when the count wraps, so that a record last written 2^32 - 1 passes ago cannot pass for a fresh one.
struct GnxEpoch { uint32_t epoch; bool clear; };
SERL_GNX_HD GnxEpoch gnx_next_epoch(uint32_t prev) {
  GnxEpoch e;
  e.clear = prev == 0u || prev == 0xffffffffu;
  e.epoch = e.clear ? 1u : prev + 1u;
  return e;
}

// Records per image that a layer of P output pixels and Cout channels can need: its tiles are at least 128 rows x 64 channels
// (LDS-DMA kernel; the row-slab kernels' are 256 x 64), and only tiles that lie in one image exchange.
SERL_GNX_HD long gnx_records_per_image(int P, int Cout) { return P % 128 == 0 ? (long)(P / 128) * (Cout / 64) : 0; }

// RECORD ADDRESSING.  A launch's tiles are numbered tile = (image * rows + row_tile) * tiles_n + column_tile (rows row tiles per
// image); the record of a tile is record `tile` of its layer's region, so no record is shared or reused within a pass.  A tile
// needs the records of the row tiles of ITS image and ITS column tile: `count` records starting at `first`, `stride` apart, its
// own being number `self` of them.
struct GnxPeers { long first; int stride, count, self; };
SERL_GNX_HD GnxPeers gnx_peers(long tile, int rows, int tiles_n) {
  const long per_image = (long)rows * tiles_n, image = tile / per_image;
  const int within = (int)(tile - image * per_image);
  GnxPeers p;
  p.first = image * per_image + within % tiles_n;
  p.stride = tiles_n;
  p.count = rows;
  p.self = within / tiles_n;
  return p;
}

}  // namespace serl
