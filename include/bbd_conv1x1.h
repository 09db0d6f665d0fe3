/*
 * bbd_conv1x1.h - the two host-side queries that go with bbd_conv1x1s2_fwd / _bwd_data / _wgrad (include/bbd_hip.h,
 * which describes the calls and their numerics).  Neither enqueues work, so neither takes a stream.  They are kept apart
 * from bbd_hip.h for the reason include/bbd_wgrad.h gives: the set of stream-less helpers of that header is a fixed part
 * of the ABI surface (tests/test_abi_surface.py).  baseboostdepth_amd/_lib.py types both from THIS file with the same
 * reader (`lib.conv1x1s2_supported`, `lib.conv1x1s2_wgrad_scratch_doubles`).
 *
 * bbd_conv1x1s2_supported             1 where the three calls take x [N, C, H, W] and a weight [K, C, 1, 1] - C and K
 *                                     multiples of 16, N, H, W >= 1, every tensor and the scratch below 2^31 elements -
 *                                     else 0
 * bbd_conv1x1s2_wgrad_scratch_doubles the doubles `scratch` of bbd_conv1x1s2_wgrad must hold for the shape (it does not
 *                                     grow with N); 0 where the shape is not taken
 */
#ifndef BBD_CONV1X1_H
#define BBD_CONV1X1_H

#ifdef __cplusplus
extern "C" {
#endif

int bbd_conv1x1s2_supported(int N, int C, int K, int H, int W);
int bbd_conv1x1s2_wgrad_scratch_doubles(int N, int C, int K, int H, int W);

#ifdef __cplusplus
}
#endif

#endif /* BBD_CONV1X1_H */
