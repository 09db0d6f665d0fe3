/*
 * bbd_wgrad.h - the two host-side queries that go with bbd_conv3x3_wgrad (include/bbd_hip.h, which describes the call,
 * its numerics and BBD_WGRAD_RUN).  Neither enqueues work, so neither takes a stream.  They are kept apart from
 * bbd_hip.h because the set of stream-less helpers of that header is a fixed part of the ABI surface
 * (tests/test_abi_surface.py); the rules of that header hold here too, and baseboostdepth_amd/_lib.py types both from
 * THIS file with the same reader (`lib.conv3x3_wgrad_supported`, `lib.conv3x3_wgrad_scratch_doubles`).
 *
 * bbd_conv3x3_wgrad_supported       1 where bbd_conv3x3_wgrad takes the shape - C and K multiples of 16 in 16..1024,
 *                                   N, H, W >= 1, every tensor and the scratch below 2^31 elements - else 0
 * bbd_conv3x3_wgrad_scratch_doubles the doubles `scratch` of that call must hold for the shape; 0 where it is not taken
 */
#ifndef BBD_WGRAD_H
#define BBD_WGRAD_H

#ifdef __cplusplus
extern "C" {
#endif

int bbd_conv3x3_wgrad_supported(int N, int C, int K, int H, int W);
int bbd_conv3x3_wgrad_scratch_doubles(int N, int C, int K, int H, int W);

#ifdef __cplusplus
}
#endif

#endif /* BBD_WGRAD_H */
