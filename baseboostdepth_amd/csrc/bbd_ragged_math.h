/* bbd_ragged_math.h - what every kernel over a ragged batch restates, shared with the host ports of the test tier
 * (tests/host_port/): the 64-bit offset that travels as two int32 words, the BBD_EVAL_DESC row, and the packed colour
 * (r | g << 8 | b << 16) of the picture kernels.  Validity rules (which rows a kernel skips) stay with the kernels. */
#ifndef BBD_RAGGED_MATH_H
#define BBD_RAGGED_MATH_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/bbd_hip.h"
#include "bbd_math.h" /* BBD_HD */

/* Offset or address from its low and high word (the Python side splits it: tables.split64). */
BBD_HD size_t bbd_join64(int32_t lo, int32_t hi) { return (size_t)(uint32_t)lo | ((size_t)(uint32_t)hi << 32); }

/* One BBD_EVAL_DESC row: element offset of the map, its size, the crop window [r0, r1) x [c0, c1). */
struct BbdEvalRow {
  size_t off;
  int GH, GW, r0, r1, c0, c1;
};

BBD_HD BbdEvalRow bbd_eval_row(const int32_t* desc, int i) {
  const int32_t* d = desc + (size_t)i * BBD_EVAL_DESC;
  BbdEvalRow m;
  m.off = bbd_join64(d[0], d[1]);
  m.GH = d[2]; m.GW = d[3]; m.r0 = d[4]; m.r1 = d[5]; m.c0 = d[6]; m.c1 = d[7];
  return m;
}

/* One row of a [rows,3] uint8 LUT as a packed colour, and the three bytes of a packed colour. */
BBD_HD uint32_t bbd_pack_rgb(const uint8_t* rgb) {
  return (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16);
}
BBD_HD void bbd_put_rgb(uint8_t* o, uint32_t c) {
  o[0] = (uint8_t)c; o[1] = (uint8_t)(c >> 8); o[2] = (uint8_t)(c >> 16);
}

#endif /* BBD_RAGGED_MATH_H */
