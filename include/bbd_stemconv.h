/*
 * bbd_stemconv.h - the two host-side queries that go with bbd_stem_conv7s2_fwd / bbd_stem_conv7s2_wgrad
 * (include/bbd_hip.h, which describes the calls and their numerics).  Neither enqueues work, so neither takes a stream.
 * They are kept apart from bbd_hip.h for the reason include/bbd_wgrad.h gives: the set of stream-less helpers of that
 * header is a fixed part of the ABI surface (tests/test_abi_surface.py).  baseboostdepth_amd/_lib.py types both from
 * THIS file with the same reader (`lib.stem_conv7s2_supported`, `lib.stem_conv7s2_wgrad_scratch_doubles`).
 *
 * bbd_stem_conv7s2_supported             1 where both calls take x [N, C, H, W] and a weight [K, C, R, S] - K = 64, C 3 or
 *                                        6, R = S = 7, N, H, W >= 1, input and output below 2^31 elements - else 0
 * bbd_stem_conv7s2_wgrad_scratch_doubles the doubles `scratch` of bbd_stem_conv7s2_wgrad must hold for the shape; 0 where
 *                                        it is not taken
 */
#ifndef BBD_STEMCONV_H
#define BBD_STEMCONV_H

#ifdef __cplusplus
extern "C" {
#endif

int bbd_stem_conv7s2_supported(int N, int C, int K, int H, int W, int R, int S);
int bbd_stem_conv7s2_wgrad_scratch_doubles(int N, int C, int K, int H, int W, int R, int S);

#ifdef __cplusplus
}
#endif

#endif /* BBD_STEMCONV_H */
