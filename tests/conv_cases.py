"""Launch cases of the 5x5 convolution (sept_conv.hip): one row per launch, together reaching every kernel instantiation
of the tile table (kConvVariants) -- every entry in every form it is instantiated in -- at its edges.

Row = (B, H, W, cin, cout, form, entry): the launch sept_conv5x5_launch_variant(B, H, W, cin, cout, form) answers `entry`
(the index in kConvVariants) for it; tests/test_conv_variants.py checks that on the CPU and tests/test_conv_variants_gpu.py
runs every row against a float64 reference.

form: 0 plain, 1 epilogue (BatchNorm statistics for forward shapes cin <= cout, BatchNorm backward sums for data-gradient
shapes cin > cout), 2 BatchNorm-apply loader (LBN), 3 LBN + backward sums, 4 activation loader (LACT), 5 LACT + statistics.

How the rows were chosen (the choice of entry is not monotone in W, so the widths come from a scan of W = 1 .. 400):
  - per instantiation, the narrowest and the widest W at which a launch takes it (different ranges of W wherever there
    are several; W <= 4, where the halo covers the whole row, wherever the kernel is reached there);
  - both launch regimes where the entry is reached in both: B = 3 (fewer than 192 workgroups: 512-pixel tiles give way
    to 256-pixel ones) and B = 193 (at least 192 workgroups at one tile per image);
  - at least three image rows (with fewer, the taps of the outer kernel rows only ever read the zero halo and a kernel
    that dropped them would pass), except in the rows that make an image smaller than one tile;
  - H * W never a multiple of the tile's pixels (a ragged last tile), and for every entry one row whose image is smaller
    than one tile; B is never a multiple of 8 (grid.y is padded to whole groups of 8 images);
  - the LBN forms (2, 3) at even H and W (whole 2x2 windows).
"""

FORM_NAMES = ("plain", "epilogue", "lbn", "lbn_sums", "act", "act_stats")
PAIRS = ((32, 64), (64, 128), (64, 32), (128, 64), (128, 128))

CASES = [  # (B, H, W, cin, cout, form, entry)
    (193, 21, 12, 32, 64, 0, 0),
    (193, 3, 267, 32, 64, 0, 0),
    (193, 21, 12, 32, 64, 1, 0),
    (193, 3, 267, 32, 64, 1, 0),
    (193, 21, 12, 32, 64, 4, 0),
    (193, 3, 267, 32, 64, 4, 0),
    (193, 21, 12, 32, 64, 5, 0),
    (193, 3, 267, 32, 64, 5, 0),
    (3, 214, 3, 32, 64, 0, 1),
    (193, 3, 313, 32, 64, 0, 1),
    (3, 214, 3, 32, 64, 1, 1),
    (193, 3, 313, 32, 64, 1, 1),
    (3, 214, 3, 32, 64, 4, 1),
    (193, 3, 313, 32, 64, 4, 1),
    (3, 214, 3, 32, 64, 5, 1),
    (193, 3, 313, 32, 64, 5, 1),
    (3, 640, 1, 32, 64, 0, 2),
    (193, 3, 324, 32, 64, 0, 2),
    (3, 640, 1, 32, 64, 1, 2),
    (193, 3, 324, 32, 64, 1, 2),
    (3, 640, 1, 32, 64, 4, 2),
    (193, 3, 324, 32, 64, 4, 2),
    (3, 640, 1, 32, 64, 5, 2),
    (193, 3, 324, 32, 64, 5, 2),
    (3, 160, 2, 32, 64, 0, 3),
    (193, 3, 153, 32, 64, 0, 3),
    (3, 160, 2, 32, 64, 1, 3),
    (193, 3, 153, 32, 64, 1, 3),
    (3, 160, 2, 32, 64, 4, 3),
    (193, 3, 153, 32, 64, 4, 3),
    (3, 160, 2, 32, 64, 5, 3),
    (193, 3, 153, 32, 64, 5, 3),
    (3, 320, 2, 64, 128, 0, 4),
    (193, 3, 292, 64, 128, 0, 4),
    (3, 320, 2, 64, 128, 1, 4),
    (193, 3, 292, 64, 128, 1, 4),
    (3, 214, 3, 64, 128, 0, 5),
    (193, 3, 313, 64, 128, 0, 5),
    (3, 214, 3, 64, 128, 1, 5),
    (193, 3, 313, 64, 128, 1, 5),
    (3, 320, 1, 64, 128, 0, 6),
    (193, 64, 1, 64, 128, 0, 6),
    (3, 320, 1, 64, 128, 1, 6),
    (193, 64, 1, 64, 128, 1, 6),
    (193, 21, 12, 64, 32, 0, 7),
    (193, 3, 267, 64, 32, 0, 7),
    (193, 21, 12, 64, 32, 1, 7),
    (193, 3, 267, 64, 32, 1, 7),
    (193, 22, 12, 64, 32, 2, 7),
    (193, 4, 266, 64, 32, 2, 7),
    (193, 22, 12, 64, 32, 3, 7),
    (193, 4, 266, 64, 32, 3, 7),
    (193, 28, 9, 64, 32, 0, 8),
    (193, 3, 277, 64, 32, 0, 8),
    (193, 28, 9, 64, 32, 1, 8),
    (193, 3, 277, 64, 32, 1, 8),
    (3, 640, 1, 64, 32, 0, 9),
    (193, 3, 324, 64, 32, 0, 9),
    (3, 640, 1, 64, 32, 1, 9),
    (193, 3, 324, 64, 32, 1, 9),
    (3, 6, 114, 64, 32, 0, 10),
    (193, 3, 329, 64, 32, 0, 10),
    (3, 6, 114, 64, 32, 1, 10),
    (193, 3, 329, 64, 32, 1, 10),
    (3, 8, 106, 64, 32, 2, 10),
    (193, 4, 328, 64, 32, 2, 10),
    (3, 8, 106, 64, 32, 3, 10),
    (193, 4, 328, 64, 32, 3, 10),
    (3, 214, 3, 64, 32, 0, 11),
    (193, 3, 313, 64, 32, 0, 11),
    (3, 214, 3, 64, 32, 1, 11),
    (193, 3, 313, 64, 32, 1, 11),
    (3, 160, 4, 64, 32, 2, 11),
    (193, 4, 312, 64, 32, 2, 11),
    (3, 160, 4, 64, 32, 3, 11),
    (193, 4, 312, 64, 32, 3, 11),
    (3, 160, 2, 64, 32, 0, 12),
    (193, 32, 2, 64, 32, 0, 12),
    (3, 160, 2, 64, 32, 1, 12),
    (193, 32, 2, 64, 32, 1, 12),
    (3, 160, 2, 64, 32, 2, 12),
    (193, 32, 2, 64, 32, 2, 12),
    (3, 160, 2, 64, 32, 3, 12),
    (193, 32, 2, 64, 32, 3, 12),
    (193, 85, 3, 128, 64, 0, 13),
    (3, 5, 267, 128, 64, 0, 13),
    (193, 85, 3, 128, 64, 1, 13),
    (3, 5, 267, 128, 64, 1, 13),
    (3, 320, 2, 128, 64, 0, 14),
    (3, 5, 138, 128, 64, 0, 14),
    (193, 64, 2, 128, 64, 0, 14),
    (3, 320, 2, 128, 64, 1, 14),
    (3, 5, 138, 128, 64, 1, 14),
    (193, 64, 2, 128, 64, 1, 14),
    (3, 80, 8, 128, 64, 0, 15),
    (3, 5, 148, 128, 64, 0, 15),
    (193, 12, 10, 128, 64, 0, 15),
    (3, 80, 8, 128, 64, 1, 15),
    (3, 5, 148, 128, 64, 1, 15),
    (193, 12, 10, 128, 64, 1, 15),
    (3, 320, 2, 128, 64, 2, 15),
    (193, 4, 148, 128, 64, 2, 15),
    (3, 320, 2, 128, 64, 3, 15),
    (193, 4, 148, 128, 64, 3, 15),
    (3, 214, 3, 128, 128, 0, 16),
    (193, 3, 104, 128, 128, 0, 16),
    (3, 214, 3, 128, 128, 1, 16),
    (193, 3, 104, 128, 128, 1, 16),
    (3, 320, 2, 128, 128, 0, 17),
    (193, 3, 138, 128, 128, 0, 17),
    (3, 320, 2, 128, 128, 1, 17),
    (193, 3, 138, 128, 128, 1, 17),
    (3, 3, 3, 32, 64, 0, 1),
    (3, 3, 1, 32, 64, 0, 2),
    (3, 3, 2, 32, 64, 0, 3),
    (3, 3, 2, 64, 128, 0, 4),
    (3, 3, 3, 64, 128, 0, 5),
    (3, 3, 1, 64, 32, 0, 9),
    (3, 2, 114, 64, 32, 0, 10),
    (3, 3, 3, 64, 32, 0, 11),
    (3, 3, 3, 128, 128, 0, 16),
    (3, 3, 2, 128, 128, 0, 17),
]


def case_id(c):
    B, H, W, cin, cout, form, entry = c
    return f"e{entry}-{FORM_NAMES[form]}-{cin}to{cout}-B{B}-{H}x{W}"
