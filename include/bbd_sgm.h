/*
 * bbd_sgm.h - the host-side query that goes with bbd_sgm_hints (include/bbd_hip.h, which describes the call).  It
 * enqueues no work, so it takes no stream.  It is kept apart from bbd_hip.h for the reason include/bbd_wgrad.h gives: the
 * set of stream-less helpers of that header is a fixed part of the ABI surface (tests/test_abi_surface.py).
 * baseboostdepth_amd/_lib.py types it from THIS file with the same reader (`lib.sgm_scratch_bytes`).
 *
 * bbd_sgm_scratch_bytes  the bytes `scratch` of bbd_sgm_hints must hold: with P = B * H * W, 2 P grey bytes and 4 P
 *                        selection bytes (each rounded up to 8), 16 P census bytes, P * D cost bytes and 2 P * D bytes of
 *                        path sums; `paths` (4 or 8) does not change it.  0 where the call refuses the shape
 */
#ifndef BBD_SGM_H
#define BBD_SGM_H

#ifdef __cplusplus
extern "C" {
#endif

long bbd_sgm_scratch_bytes(int B, int H, int W, int D, int paths);

#ifdef __cplusplus
}
#endif

#endif /* BBD_SGM_H */
