"""The transform lengths of the acquisition FFT sweep (tests/test_gpu_acq_surfaces.py) and what tests/test_acq_fft_plan_cpu.py
asserts about the plans they get (csrc/acq_fft.hip: make_plan, factor, choose_cols).  The list is short on purpose; the planner test
states the coverage it must reach, so a change of the planner that loses a stage position fails there, not silently on the GPU."""

# mostly below 10 000 points: every radix of {2, 3, 4, 5, 6, 8} in every stage position it can take in both passes, single-stage
# and four-stage passes, n1 == 1, n1 != n2, tiles that do not divide the vector count
SWEEP_SMALL = [2, 3, 5, 6, 8, 15, 20, 30, 36, 60, 64, 100, 240, 243, 360, 486, 625, 729, 750, 1000, 1024, 1250, 1296, 1500, 2000,
               2500, 3000, 3125, 4096, 4374, 5000, 5184, 6144, 6400, 7776, 8000, 8192, 9216, 10000, 15625, 36864, 262144]
# the FFT sizes of the reference's default front ends with their specialised shapes n1 x n2 (launch_pass: GC_CT_SHAPE; make_plan: kSplit)
PRODUCTION = {36000: (180, 200), 24000: (150, 160), 144000: (375, 384), 72000: (250, 288), 360000: (600, 600), 320000: (320, 1000)}
# their radices as GC_CT_SHAPE lists them: (columns pass, rows pass)
PRODUCTION_SHAPES = {36000: ([6, 6, 5], [8, 5, 5]), 24000: ([6, 5, 5], [8, 5, 4]), 144000: ([5, 5, 5, 3], [8, 8, 6]),
                     72000: ([5, 5, 5, 2], [8, 6, 6]), 360000: ([6, 5, 5, 4], [6, 5, 5, 4]), 320000: ([8, 8, 5], [8, 5, 5, 5])}
LARGEST = 1 << 22        # 2048 x 2048: the largest plan make_plan accepts
SWEEP = SWEEP_SMALL + list(PRODUCTION) + [LARGEST]
# refused: a prime factor of 7 or more; n2 > 2048 (kMaxPassLen)
REFUSED_PRIME = [7, 14, 77, 3584, 32736, 5172, 11 * 4096, 13 * 3125]
REFUSED_LONG = [1 << 23, 3 * (1 << 22), 8 * 5 ** 9]
