/*
 * bbd_up2conv.h - the two host-side queries that go with bbd_up2conv3x3_fwd / bbd_up2conv3x3_bwd (include/bbd_hip.h,
 * which describes the calls and their numerics).  Neither enqueues work, so neither takes a stream.  They are kept apart
 * from bbd_hip.h for the reason include/bbd_wgrad.h gives: the set of stream-less helpers of that header is a fixed part
 * of the ABI surface (tests/test_abi_surface.py).  baseboostdepth_amd/_lib.py types both from THIS file with the same
 * reader (`lib.up2conv3x3_supported`, `lib.up2conv3x3_scratch_doubles`).
 *
 * bbd_up2conv3x3_supported       1 where both calls take the shape - C = K = 16, N, h, w >= 1, the output
 *                                [N, K, 2h, 2w] below 2^31 elements - else 0
 * bbd_up2conv3x3_scratch_doubles the doubles `scratch` of bbd_up2conv3x3_bwd must hold for the shape (one per channel and
 *                                source row of the batch); 0 where the shape is not taken
 */
#ifndef BBD_UP2CONV_H
#define BBD_UP2CONV_H

#ifdef __cplusplus
extern "C" {
#endif

int bbd_up2conv3x3_supported(int N, int C, int K, int h, int w);
int bbd_up2conv3x3_scratch_doubles(int N, int C, int K, int h, int w);

#ifdef __cplusplus
}
#endif

#endif /* BBD_UP2CONV_H */
