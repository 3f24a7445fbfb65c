"""The conversions the resampler's launch-shape tests run (tests/test_resample_geometry_cpu.py pins what each reaches on the
host, tests/test_gpu_resample_shapes.py runs each through the kernel): (orig, new, lowpass_filter_width, rolloff) and the part
of csrc/resample.hip the case is there for.  With g = gcd, o = orig / g, n = new / g, K = 2 ceil(lpw o / (min(o, n) rolloff)) + o."""

CASES = [
    # ---- phase slices: gridDim.y > 1, pbase > 0, the guards of a ragged last slice
    ((47952, 44100, 6, 0.99), "48 kHz NTSC pull-down to 44.1 kHz: o 1332, n 1225, K 1346; two ragged slices of 613 + 612 phases, one "
                              "frame group, a window of 10670 floats"),
    ((44100, 47952, 6, 0.99), "the way back: n 1332, two even slices of 666, lanes 167 (668 slots: q < pn bites in both)"),
    ((11025, 96000, 6, 0.99), "n 1280: two even slices of 640 with lanes 160, no idle slot at all"),
    ((1000, 2049000, 6, 0.99), "o 1, n 2049: three slices of 683; 4 x 171 = 684 slots, so q < pn bites in every slice"),
    ((4000, 132300, 6, 0.99), "n 1323, pn 662, lanes 166 (664 slots): q < pn and pbase + q < n both bite in the last slice of 661"),
    # ---- the PH switch at n = 32
    ((1000, 31000, 6, 0.99), "n 31: the largest PH = 1 shape, 31 lanes of real work, 8 frame groups"),
    ((1000, 32000, 6, 0.99), "n 32: the smallest PH = 4 shape, lanes 8, every slot live"),
    ((1000, 33000, 6, 0.99), "n 33: PH = 4 with lanes 9, 36 slots for 33 phases"),
    ((8000, 48000, 6, 0.99), "n 6: PH = 1 with more than three lanes"),
    ((48000, 32000, 6, 0.99), "o 3, n 2: PH = 1, two lanes, 128 frame groups"),
    # ---- the tap tiling
    ((22050, 44100, 1, 0.99), "lowpass_filter_width 1: K 5 < 8, no prefetched tile, the tail loop does every tap"),
    ((48000, 8000, 6, 0.99), "K 80: a multiple of 8, no tail loop; n 1"),
    ((5000, 220500, 6, 0.99), "K 24: a multiple of 8 with n 441"),
    # ---- the window limit
    ((48000, 100, 6, 0.99), "o 480, K 6300: one frame group, a window of 9660 of 12288 floats; n 1, so one lane per frame"),
    ((96000, 11025, 6, 0.99), "o 1280, n 147, K 1386: one frame group, a window of 10346"),
    # ---- two shipped conversions as anchors
    ((16000, 44100, 6, 0.99), "shipped: o 160, n 441, K 174"),
    ((44100, 16000, 6, 0.99), "shipped: o 441, n 160, K 475; 40 lanes allow 6 frame groups, the window cuts them to 3"),
    # ---- pick_groups with want > 1 (want = n_frames / 6144, so m 6144 o input samples).  The cases above reach it too where
    # they have more than one frame group: 1000 -> 31000 goes from 2 to 4 groups at 18432 input samples
    ((48000, 16000, 6, 0.99), "shipped: o 3, n 1, K 41; one lane, so 55 groups fill a wave to 85 % and only want = 56 changes the "
                              "launch (1.03 M input samples)"),
    ((44100, 48000, 6, 0.99), "shipped: o 147, n 160, K 161; 40 lanes, up to 6 frame groups; launch groups 3 -> 6 at "
                              "want = 4 (3.6 M input samples)"),
]

# (orig, new, lpw, rolloff) jat_resampler_create refuses because no block shape keeps the staged window within 12288 floats,
# with the window 7 o + K of the smallest shape (one frame group)
REFUSED = [
    ((96000, 100, 6, 0.99), 7 * 960 + 12598),
    # o 2671 (a prime), n 14700, K 2685: a table of 39.5 M entries is under the 2^26 limit, the window of 21382 does not fit
    ((8013, 44100, 6, 0.99), 7 * 2671 + 2685),
]

IDS = [f"{c[0]}-{c[1]}" + (f"-lpw{c[2]}" if c[2] != 6 else "") for c, _ in CASES]
