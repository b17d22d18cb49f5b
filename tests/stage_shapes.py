"""Launch shapes of the GPU tests of the CNN stage kernels (test_gpu_nnet.py, test_gpu_stage32_pm.py).  They live here so that the
host test of the launch plans (test_stage_plans_host.py) can check, without a GPU, that together they reach every kernel instantiation
of every launch table."""

# rp_nn_resstage16: (B, H, W)
# images above 128 pixels run one workgroup per image (k_resstage16_wg: 4 or 8 waves share the tiles): 25x25 is the 50x50 board's
# 10x10 (96 + 4 pixels), 9x11 (96 + 3) and 7x14 (96 + 2) take their last pixels through the 4x4x1 tail blocks
# (8000 leaves of 5x5: four leaves per wave = 96 + 4 pixels: a tail tile across images)
RESSTAGE16 = [(5, 10, 10), (1030, 10, 10), (6, 9, 11), (5, 7, 14), (8000, 5, 5), (64, 7, 9), (33, 3, 3), (17, 8, 8), (9, 5, 5), (3, 1, 1), (21, 11, 11), (6, 8, 16), (7, 5, 13),
              (5, 25, 25), (530, 25, 25), (3, 20, 32), (4, 12, 12), (2, 16, 20), (3, 9, 33), (2, 21, 17),
              # the tile counts that no shape above reaches: 3, 6 without tail blocks, 7 (102 pixels: a tail of 6); 4 tiles on 4 and on 8 waves
              (7, 3, 11), (5, 9, 9), (5, 6, 17), (3, 14, 15), (3, 20, 21)]

# rp_nn_resstage32: (B, H, W), each for both 32-channel stages
# above 80 pixels: several leaves per WORKGROUP (k_resstage32_wg); 13x13 is the 50x50 board's second stage
RESSTAGE32 = [(5, 5, 5), (1030, 5, 5), (3001, 3, 3), (7, 3, 3), (64, 4, 4), (33, 2, 3), (3, 1, 1), (10, 8, 8), (11, 7, 9), (4, 8, 10), (13, 6, 6),
              (7, 13, 13), (1000, 13, 13), (5, 10, 10), (3, 16, 16), (2, 22, 23), (4, 9, 11), (5, 12, 20),
              (3, 16, 17)]  # 17 tiles: 3 on each of 8 waves

# rp_nn_convpool32: (Cin, B, H, W)
CONVPOOL32 = [(16, 5, 10, 10), (16, 1030, 10, 10), (16, 6, 9, 11), (16, 5, 7, 14), (16, 8000, 5, 5), (16, 33, 7, 9),  # 10x10 / 9x11 / 7x14: 96 pixels + a 4x4x1 tail of 4 / 3 / 2
              (16, 9, 3, 3), (16, 4, 1, 1), (16, 21, 8, 13), (16, 64, 4, 4),
              (32, 5, 5, 5), (32, 1030, 5, 5), (32, 3001, 3, 3), (32, 17, 8, 8), (32, 11, 7, 9), (32, 6, 2, 5), (32, 3, 1, 1), (32, 10, 8, 10),
              # above 112 / 80 pixels: k_convpool32_wg (25x25x16 -> 13x13x32 and 13x13x32 -> 7x7x32 at the 50x50 board)
              (16, 5, 25, 25), (16, 300, 25, 25), (16, 3, 12, 12), (16, 4, 20, 31), (16, 2, 9, 33), (32, 7, 13, 13), (32, 500, 13, 13), (32, 4, 16, 16),
              (32, 3, 22, 23), (32, 5, 10, 10), (32, 2, 9, 11),
              # the remaining instantiations: 2, 3, 5, 6 tiles per wave at Cin 16 and 3 at Cin 32; workgroups of 4 x 2, 4 x 4, 8 x 4 (Cin 16), 8 x 3 tiles (Cin 32)
              (16, 7, 3, 6), (16, 7, 3, 11), (16, 5, 5, 13), (16, 5, 9, 9), (32, 7, 3, 11), (16, 3, 11, 11), (16, 3, 14, 15), (16, 3, 20, 21), (32, 3, 16, 17)]

# position-major rp_nn_resstage32 (RP_STAGE32_PM forced on and off), S x S images: batches per S
# short last task, exactly one task, one leaf into the next task, more tasks than one round of a small grid
STAGE32_PM_BATCHES = {3: (1, 15, 16, 17, 33, 1030), 5: (1, 15, 16, 17, 65, 1030)}

# position-major rp_nn_convpool32 (RP_CONVPOOL_PM forced on and off), 32 -> 32 channels on 5x5: short task, one leaf short of a task,
# exactly one, one into the next, a short last task, two tiles per wave of the pixel-major kernel
CONVPOOL32_PM_BATCHES = (1, 15, 16, 17, 65, 1030)
# position-paired rp_nn_resstage16 (RP_STAGE16_PP forced on and off) on 10x10: tasks of eight leaves; the last batch gives a workgroup
# of a 256-CU device a second task (stage16_pp_worker.BATCHES)
STAGE16_PP_BATCHES = (1, 7, 8, 9, 23, 8 * 512 + 3)

ENTRY_RESSTAGE16, ENTRY_CONVPOOL32, ENTRY_RESSTAGE32 = 0, 1, 2  # rp_debug_stage_plan's entry
KNOB_OF_ENTRY = ("RP_STAGE16_PP", "RP_CONVPOOL_PM", "RP_STAGE32_PM")  # read at every call: 0 = the pixel-major kernel, 1 = the newer one


def row_limit_cases():
    """The launches of test_gpu_stage_rows.py: (entry, Cin, B, H, W, knob) with every shape above under knob 0 and, where the newer
    family takes the image size (10x10 at 16 channels, 5x5 at 32 -> 32, 3x3 and 5x5 at the 32-channel stages), under knob 1 as well.
    test_stage_plans_host.py checks that they reach every kernel instantiation."""
    cases = []
    for (B, H, W) in RESSTAGE16 + [(B, 10, 10) for B in STAGE16_PP_BATCHES]:
        cases += [(ENTRY_RESSTAGE16, 16, B, H, W, k) for k in ((0, 1) if (H, W) == (10, 10) else (0,))]
    for (cin, B, H, W) in CONVPOOL32 + [(32, B, 5, 5) for B in CONVPOOL32_PM_BATCHES]:
        cases += [(ENTRY_CONVPOOL32, cin, B, H, W, k) for k in ((0, 1) if (cin, H, W) == (32, 5, 5) else (0,))]
    for (B, H, W) in RESSTAGE32 + [(B, S, S) for S, batches in STAGE32_PM_BATCHES.items() for B in batches]:
        cases += [(ENTRY_RESSTAGE32, 32, B, H, W, k) for k in ((0, 1) if (H, W) in ((3, 3), (5, 5)) else (0,))]
    return list(dict.fromkeys(cases))
