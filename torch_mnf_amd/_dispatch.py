"""Which kernel family a layer call takes: every shape / row-count threshold of the Python layer in one place, and the
rule that reads them -- the routes the Python layer decides by itself (MAF / IAF, NSF_AR, the wide AffineHalfFlow
gradients) are the rows of RT_ROUTES, decided by rt_route() alone: the layers' predicates in flows.py and tier() both ask it.

The C library picks among its kernels by SHAPE (a specialised kernel where the shape has one, else the run-time-shaped
matrix-core kernels of csrc/mnf_rt.h, else the VALU any-shape kernels); what is decided here is by ROW COUNT -- where a
faster-per-row kernel does not pay for its extra launches yet -- plus the test / measurement switches.  INTEGRATION.md
("Which kernel runs") is this table in prose; tools/coverage_map.py measures it; tests set these attributes directly
(``monkeypatch.setattr(torch_mnf_amd._dispatch, "NSF_PAD_MIN_ROWS", 0)``).  Environment switches of the package, all of
them: MNF_LIB_PATH (another build of the library), MNF_DETERMINISTIC (fixed-order gradient sums; read by the library),
MNF_FP32_MFMA (fp32 instead of split-f16 matrix-core arithmetic), MNF_CHECK_PARAMS (stale-image detector),
MNF_NO_RUN_FUSION and MNF_NO_PAIR_FUSION (layer-by-layer passes, for per-layer measurements).

| layer (direction)        | rows            | shape                                             | kernel family                  |
|--------------------------|-----------------|---------------------------------------------------|--------------------------------|
| AffineHalfFlow fwd       | any             | 3 hidden layers <= 32 (64 at d = 32/64/128), d <= 256 | ahf_split(_stack) / ahf_mfma |
|                          | >= RT_MIN_ROWS  | any h_sizes (>= 1 layer, widths 4..256), any d    | ahf_rt                         |
|                          | >= RT_MIN_ROWS, no grad | a run of 2..32 such layers of one shape   | ahf_stack_rt (one launch)      |
|                          | else            | anything                                          | ahf_generic (VALU)             |
| AffineHalfFlow bwd       | >= BWD_SPLIT_MIN_ROWS | the split kernel's shapes                   | ahf_bwd_split                  |
|                          | any             | the fp32-MFMA kernel's shapes                     | ahf_bwd_mfma_fp32              |
|                          | >= RT_MIN_ROWS  | 1..4 hidden layers of widths 4..64, any d         | ahf_bwd_rt                     |
|                          | >= RT_MIN_ROWS, fuse_rt_training | a run of 2..32 such layers of one shape | ahf_bwd_stack_rt (one launch) |
|                          | >= AHF_BWD_RT_WIDE_MIN_ROWS (opt-in: None) | 1..4 hidden layers, widest 65..128, any d (runs too) | ahf_bwd_rt / ahf_bwd_stack_rt |
|                          | else            | anything                                          | ahf_bwd_generic                |
| NSF_CL fwd               | any             | d % 8 == 0 up to 64, n_h <= 16, K 5/8 (10: d<=32) | nsf_mfma_split                 |
|                          | >= NSF_PAD_MIN_ROWS | other d <= 64 (zero-padded twin layer)        | nsf_mfma_split                 |
|                          | >= RT_MIN_ROWS  | any d, K 2..16, hidden widths 4..64               | nsf_rt                         |
|                          | else            | anything                                          | nsf_generic                    |
| NSF_CL bwd               | any             | the tile kernel's shapes                          | nsf_bwd_tile (+ fix-up)        |
|                          | >= RT_MIN_ROWS  | any d, K 2..16, 1..4 layers 4..64, LDS slot (*)   | nsf_bwd_rt                     |
|                          | else            | anything                                          | nsf_bwd_generic                |
| RNVP fwd                 | few (C side)    | one hidden layer <= 64                            | rnvp_few                       |
|                          | any             | one hidden layer <= 64, d >= 49                   | rnvp_resident / narrow / split |
|                          | >= RT_MIN_ROWS  | any number of layers of widths 4..256, any d      | rnvp_rt                        |
|                          | else            | anything                                          | rnvp_generic                   |
| RNVP bwd                 | few             | one hidden layer <= 64                            | rnvp_bwd_few                   |
|                          | not rnvp_bwd_small() | one hidden layer <= 64, padded d >= 64       | rnvp_bwd_mfma                  |
|                          | >= RT_MIN_ROWS  | 1..4 layers of widths 4..128, any d               | rnvp_bwd_rt                    |
|                          | else            | anything                                          | rnvp_bwd_generic               |
| Glow fwd / inv / bwd-x   | any             | d = 16 / 32 / 64 / 128                            | linear_rows_mfma               |
|                          | >= GLOW_RT_MIN_ROWS | any other 2 <= d <= 1024                      | linear_rows_rt                 |
|                          | else            | anything                                          | linear_rows_generic (VALU)     |
| Glow bwd-W               | any             | d = 32                                            | xtg32_mfma_kernel              |
|                          | >= GLOW_RT_MIN_ROWS | any other 2 <= d <= 1024 (64 and 128 too)     | linear_rows_bwd_weight_rt      |
|                          | else            | anything                                          | xtg_kernel (VALU, atomics)     |
| [Glow, ActNorm].inverse, training fwd | any | d = 16 / 32 / 64                                 | glow_actnorm_inv               |
|                          | GLOW_ACTNORM_RT (opt-in), where Glow is on linear_rows_rt | other 2 <= d <= 1024 but 128 | glow_actnorm_inv_rt |
| [Glow, ActNorm].inverse, training bwd | any | d = 16 / 32 / 64                                 | glow_actnorm_inv_bwd           |
|                          | GLOW_ACTNORM_RT (opt-in), where Glow is on linear_rows_rt | other 2 <= d <= 1024 but 128 | glow_actnorm_inv_bwd_rt |
| MAF.inverse / IAF.forward fwd | >= MAF_RT_MIN_ROWS | >= 1 hidden layer of widths 4..128, any d     | maf_rt                         |
|                          | else            | anything                                          | maf_generic (VALU)             |
| MAF.inverse / IAF.forward bwd | >= MAF_RT_MIN_ROWS | 1..4 hidden layers of widths 4..64, any d     | maf_bwd_rt                     |
|                          | else            | anything                                          | maf_bwd_generic (VALU, atomics) |
| MAF.forward / IAF.inverse fwd | >= MAF_SEQ_RT_MIN_ROWS | maf_rt's shapes whose net stays resident in LDS   | maf_seq_rt                     |
|                          | else            | anything (element by element)                     | maf_generic (VALU)             |
| MAF.forward / IAF.inverse bwd | >= MAF_SEQ_BWD_RT_MIN_ROWS (opt-in: None) | maf_bwd_rt's shapes whose solve plan fits LDS | maf_seq_bwd_rt |
|                          | else            | anything (element by element)                     | maf_bwd_generic (VALU, atomics) |
| NSF_AR.inverse fwd       | >= NSF_AR_RT_MIN_ROWS (opt-in: None) | d >= 2, K 2..16, 1..4 hidden layers of widths 4..16 | nsf_ar_rt |
|                          | else            | anything                                          | nsf_ar_generic (VALU)          |
| NSF_AR.inverse bwd       | >= NSF_AR_BWD_RT_MIN_ROWS (opt-in: None) | nsf_ar_rt's shapes with K = 5 or 8      | nsf_ar_bwd_rt                  |
|                          | else            | anything                                          | nsf_ar_bwd_generic (VALU, atomics) |
| NSF_AR.forward fwd       | >= NSF_AR_SEQ_RT_MIN_ROWS (opt-in: None) | 2 <= d <= 128, K = 5 or 8, 1..4 hidden layers of widths 4..16 | nsf_ar_seq_rt |
|                          | else            | anything (element by element)                     | nsf_ar_generic (VALU)          |
| NSF_AR.forward bwd       | any             | anything (element by element)                     | nsf_ar_bwd_generic (VALU, atomics) |
| NormalizingFlowModel.sample(seed=) | any    | the model is ONE run of AffineHalfFlow layers on ahf_split_stack's full-tile shapes (d / 2 in 16/32/64/128) | ahf_split_stack_sample (one launch, noise in-kernel) |
|                          | >= RT_SAMPLE_MIN_ROWS (opt-in: None) | the model is ONE run of AffineHalfFlow layers on ahf_rt / ahf_stack_rt (no gradients wanted) | ahf_rt_sample / ahf_stack_rt_sample (one launch, noise in-kernel) |
|                          | else            | anything (StandardNormal base)                    | mnf_normal_rows' noise launch, then forward's rows above without intermediates |
| sample(seed=, return_log_prob=True) | any   | as the one-launch row above, no gradients wanted  | ahf_split_stack_sample_lq (one launch: x and log_q) |
|                          | >= RT_SAMPLE_MIN_ROWS (opt-in: None) | as the ahf_stack_rt_sample row above, no gradients wanted | ahf_rt_sample_lq / ahf_stack_rt_sample_lq (one launch: x and log_q) |
|                          | else            | anything (StandardNormal base); any model when gradients are wanted | mnf_normal_rows_sq (noise + |z|^2), forward's rows above without intermediates, mnf_gauss_logq_sq |
| MNFConv2d.forward        | MNF_CONV_FUSED (opt-in: False) | n_out <= 64, n_in k^2 <= 4096          | mnf_conv_fwd (one launch behind the operands) |
|                          | else            | anything                                          | MIOpen convolutions between the library's operand and noise launches |
| MNFConv2d.forward bwd    | MNF_CONV_BWD_FUSED (opt-in: False), on mnf_conv_fwd's node | weights: mnf_conv_fwd's shapes; input: those with n_in <= 64, n_out k^2 <= 4096 | mnf_conv_bwd_weight / mnf_conv_bwd_input |
|                          | else            | anything                                          | mnf_mnf_noise_bwd, then aten's convolution_backward twice |

The *_rt rows' shape limits are the library's queries (mnf_*_rt_supported, include/mnf_hip.h), which tier() asks.  (*) The
NSF_CL gradient kernel's weight slot must stay within 40 LDS blocks and fit 160 KB with the rest: with n_h units per
layer, K <= 8 takes n_h <= 64; K = 9 n_h <= 64 at 1-2 layers, 48 at 3-4; K = 10..12 n_h <= 48 / 32; K = 13..16 n_h <= 32.

The [Glow, ActNorm].inverse rows are flows._pair_route: the pair of every [ActNormFlow, Glow, NSF_CL] block on the way
x -> z with gradients wanted, one autograd node and one launch each way (plus the fixed-order reduction of its sums;
the rt rows only with GLOW_ACTNORM_RT = True, default False: not yet measured against the layer-by-layer route);
without gradients, under MNF_NO_PAIR_FUSION=1 or with glow.force_generic = 1 (2 at the per-shape dims) the two layers
run one after the other as the Glow rows say -- as they do at d = 128, where Glow's product has a per-shape kernel
(glow_route answers "per-shape") and the pair none: only glow.force_generic = 2 sends that dim to the rt pair.

The ahf_stack_rt row is flows._AffineRun's second route (mnf_affine_half_rt_stack): a run of equal-shaped AffineHalfFlow
layers without operand image, inside a NormalizingFlow or FusedAffineStack, under wants_rt() for every layer and with no
gradients wanted -- every intermediate and log_det bit for bit those of one ahf_rt launch per layer, plus the log-prob
epilogue when the run closes a density pass.  With gradients wanted the layers run one by one as the rows above say --
unless the owner's opt-in switch ``fuse_rt_training`` (NormalizingFlow / FusedAffineStack, default False) is on: the run
is then ONE autograd node (flows._AffineRunFn), ahf_stack_rt forward with every output kept and ONE ahf_bwd_stack_rt
launch backward (mnf_affine_half_bwd_rt_stack; its fixed-order form under MNF_DETERMINISTIC=1), the last layer's
cotangents formed in the kernel when the run is a whole log_prob pass.  tier() is unchanged by the switch.

The sample(seed=) rows are NormalizingFlowModel.sample with a seed (no row-count threshold; without a seed it is torch.randn
and forward, as ever): rows first_row .. first_row + n - 1 of forward(z), z[r, c] = z0_normal(seed, r, c).  The one-launch
row needs the run on the split per-shape route with its images ready (no force_generic, no fp32 request, run fusion on, no
per-launch event marks) and mnf_affine_half_stack_sample_supported(); both rows compute the same sample, and a model takes
the same row at every call of one shape.  With return_log_prob=True the same choice is made with
mnf_affine_half_stack_sample_logq_supported() (the same shapes); log_q[r] = log N(z_r) - log_det_forward(z_r) comes out of
the stack launch, or on the general row from |z|^2 (summed in the noise launch's registers) and forward's log_det.  A call
with grad mode on and a parameter that requires grad takes the general row whatever the model: the pass then runs through
the layers' autograd nodes (there is no gradient kernel for the one launch), with gauss_logq_sq's formula as tensor ops.

The RT_SAMPLE_MIN_ROWS rows are the same two calls for a model whose run is on the run-time-shaped tier (ready_for answers
("rt", parameters): rt_route's conditions, so never below RT_MIN_ROWS unless every layer has force_generic = 2): from
RT_SAMPLE_MIN_ROWS rows on the call is ONE mnf_affine_half_rt_stack_sample(_logq) launch, the first layer's rows generated in
the kernel's registers, where mnf_affine_half_rt_stack_sample_supported() has the shape; x is bit for bit the general row's.

Two requests override the shape: an fp32 request (layer.force_fp32_mfma / MNF_FP32_MFMA=1) never lands on the *_rt
kernels, whose arithmetic is split-f16 -- it takes the fp32 matrix-core kernel where the shape has one (AffineHalfFlow and
RNVP: wherever a split kernel exists; NSF_CL: the K = 8 shapes, plain layer only), else the VALU kernel.  Under
MNF_DETERMINISTIC=1 the *_bwd_rt shapes run the same kernels in their fixed-order form (mnf_*_bwd_rt_det: a slot per
workgroup, added up in order; same kernel family names, same tiers); the VALU gradient kernels stay atomic and warn once
per layer and shape (_lib.note_atomic_sums).
layer.force_generic = 1 / 2 forces the VALU / the run-time-shaped kernels (tests, tools/coverage_map.py).
"""
from dataclasses import dataclass

# The run-time-shaped matrix-core kernels (csrc/mnf_rt.h: any layer count and widths) take a call without a per-shape
# kernel from this many rows on; below, the VALU any-shape kernels (a workgroup per few rows) have the lower latency.
# csrc/mnf_host.h kRtMinRows is the same number for the forward entry points.
RT_MIN_ROWS = 2048

# AffineHalfFlow gradients: the split-f16 kernel needs three small launches more per backward pass (gradient scale,
# operand repack, fix-up list) than the fp32-MFMA one and only pays them back from ~32k rows on (4,096 rows: 0.84 vs 0.65
# ms per 9-layer training step; 32,768: 0.72 vs 0.65; 65,536: 0.73 vs 0.75; 2^20: 4.7 vs 6.5)
BWD_SPLIT_MIN_ROWS = 49152
BWD_FP32 = False  # measurements: AffineHalfFlow gradients on the fp32-MFMA kernel at every row count

# NSF_CL with halves that are not whole float4 groups (dim = 2, 6, 10, ...) runs the per-shape matrix-core kernels on a
# zero-padded twin layer from this many rows on (NSF_CL._run_padded; tools/time_nsf_padded_twin.py, dim = 2, K = 8,
# n_h = 16, forward + backward, twin vs any-shape kernels: 690 vs 416 us at 16,384 rows, 705 vs 1,119 at 65,536)
NSF_PAD_MIN_ROWS = 49152
NSF_BWD_KERNEL = "tile"  # "generic": tests / measurements run the VALU gradient kernel where the tile kernel exists

# RNVP gradients.  The per-shape matrix-core pass (four launches) from these rows / dims on (d = 800: 227 vs 252 us at 128
# rows, 284 vs 837 us at 2,048; d = 100: 326 vs 403 us at 4,096 rows; d = 50 / 64 level at 16,384 rows, 457 vs 562 / 659
# at 32,768: tools/time_rnvp_bwd_small_dim.py)
RNVP_BWD_MFMA_MIN_ROWS = 64
RNVP_BWD_MFMA_MIN_DIM = 128
RNVP_BWD_MFMA_MID_DIM, RNVP_BWD_MFMA_MID_ROWS, RNVP_BWD_MFMA_ANY_DIM_ROWS = 96, 4096, 24576
RNVP_KEEP_Y_MIN_ROWS = 4096    # the forward pass keeps y = net(mask z) for the gradient pass from this many rows on
RNVP_BWD_GENERIC = False       # measurements: the VALU gradient kernel
RNVP_BWD_FEW_GRID_OFF = False  # tests: the matrix-core / VALU gradient kernels at every row count

# Glow's row transform x @ W (forward, inverse, grad_x) and its weight gradient x^T g: the run-time-shaped fp32
# matrix-core kernels (csrc/mnf_linear_mfma.hip: any 2 <= dim <= 1024) take a call without a per-shape kernel from this
# many rows on -- the smallest of the measured row counts (512 / 2,048 / 8,192 / 65,536 at dim 6, 48, 100, 256) from
# which they are not slower than the VALU kernels on ALL three passes (tools/time_glow_rt.py, profiles/r9/glow_rt_ab.txt).
# Forward and grad_x win from 512 rows on (dim 48 at 8,192 rows: 1.3 against 14.6 ns per row); what sets the number is
# the weight gradient, whose four launches (sums, zero, two reduction steps: ~25 us) lose to the VALU kernel's one at
# 8,192 rows and dim 6 / 48 (2.9 against 1.3, 3.8 against 1.8 ns per row) and win at 65,536 (0.44 / 0.65, 0.78 / 2.4).
GLOW_RT_MIN_ROWS = 65536

# [Glow, ActNorm].inverse as one launch each way on the run-time-shaped kernels (flows._pair_route):
# OPT-IN.  The fused pair has not been timed against the layer-by-layer route yet (tools/time_glow_actnorm_rt.py writes
# profiles/r10/glow_actnorm_rt_ab.txt), and every default route in this file rests on a measurement, so the default
# stays layer by layer; True sends the pair there wherever Glow's own product is on linear_rows_rt.  A layer's
# force_generic = 2 asks for the run-time-shaped kernels by name and takes the pair either way.
GLOW_ACTNORM_RT = False

# MAF / IAF, the one-pass direction (MAF.inverse, IAF.forward) and its gradients on the run-time-shaped matrix-core
# kernels (csrc/mnf_maf_rt.hip, mnf_maf_bwd_rt.hip; flows.MAF._rt): from this many rows on -- the smallest of
# the measured row counts (2,048 / 8,192 / 65,536 / 262,144 at (dim, hidden) = (2, 24x3), (6, 16x2), (64, 24x3), (64, 64x2))
# at which they are not slower than the VALU kernel on ALL three passes (forward, backward, forward + backward) for every
# timed shape, and never below RT_MIN_ROWS (tools/time_maf_rt.py, profiles/r14/maf_rt_ab.txt).  They win every cell, the
# narrowest one being (6, 16x2) forward + backward at 65,536 rows, 3.7 against 4.1 ns per row (at 2,048 rows: 90 against 129);
# (64, 64x2) at 262,144 rows: 0.47 against 49 forward, 4.8 against 543 backward.  The fifth timed shape, (256, 64), has no VALU kernel to compare with (its masked
# weights do not fit mnf_maf's 144 KB of LDS): from this many rows on it runs, below it is refused as before.  None would
# mean opt-in: only a layer's force_generic = 2 reaches the kernels.
MAF_RT_MIN_ROWS = 2048

# MAF / IAF, the element-by-element direction (MAF.forward, IAF.inverse: sampling from a MAF, the density of an IAF) on the
# matrix-core kernel maf_seq_rt (csrc/mnf_maf_rt.hip; flows.MAF._rt_seq), forward launches only: by the rule
# above MAF_RT_MIN_ROWS -- the smallest of the measured row counts (2,048 / 8,192 / 65,536 at (dim, hidden) = (2, 24x3),
# (6, 16x2), (64, 24x3), (64, 64x2)) from which it is not slower than the VALU kernel for every timed shape, never below
# RT_MIN_ROWS (tools/time_maf_seq_rt.py, profiles/r15/maf_seq_rt_ab.txt).  It wins every cell, the narrowest one being
# (6, 16x2) at 65,536 rows, 1.13 against 1.99 ns per row (at 2,048 rows: 25 against 63); (64, 64x2) at 65,536 rows: 10.8
# against 1,575.  None would mean opt-in: only a layer's force_generic = 2 reaches the kernel.
MAF_SEQ_RT_MIN_ROWS = 2048

# MAF / IAF, the gradients of the element-by-element direction (what an IAF is trained through: IAF.inverse is its density
# pass) on the matrix cores (csrc/mnf_maf_seq_bwd_rt.hip, family maf_seq_bwd_rt; flows.MAF._rt_seq_bwd, DESIGN.md 3.8g: a
# triangular solve for the total cotangents, then the one-pass direction's weight pass maf_bwd_rt at the decoded output):
# OPT-IN (RT_ROUTES "maf_seq_bwd"; existing tests pin maf_bwd_generic under force_generic = 2).  Under MNF_DETERMINISTIC=1
# the route runs mnf_maf_seq_bwd_rt_det (no atomic sums).  Measured (tools/time_maf_seq_bwd_rt.py, profiles/r16/maf_seq_bwd_rt_ab.txt: forward + backward, this route against
# maf_bwd_generic, at (dim, hidden) = (2, 24x3), (6, 16x2), (64, 24x3), (64, 64x2) and 2,048 / 8,192 / 65,536 rows, the fixed-order
# form too at 65,536): the route wins every cell, the narrowest being (2, 24x3) at 2,048 rows, 212 against 288 ns per row;
# (64, 64x2) at 65,536 rows: 29.3 against 11,990.  The smallest row count from which it wins every cell is 2,048 = RT_MIN_ROWS:
# the value a follow-up that may edit the pinned tests would make the default.
MAF_SEQ_BWD_RT_MIN_ROWS = None

# NSF_AR, the one-pass direction (NSF_AR.inverse: x -> z, what log_prob and training run through) on the matrix-core kernel
# nsf_ar_rt (csrc/mnf_nsf_ar_rt.hip; flows.NSF_AR._rt), forward launches only: None as shipped, so
# only a layer's force_generic = 2 reaches the kernel (RT_ROUTES "nsf_ar", by name; an existing test runs this direction above
# RT_MIN_ROWS and pins the VALU kernel).  Measured (tools/time_nsf_ar_rt.py, profiles/r17/nsf_ar_rt_ab.txt: NSF_AR.inverse
# through the layer, nsf_ar_rt against nsf_ar_generic, at (dim, K, n_h) = (2, 8, 16), (6, 5, 8), (16, 8, 8), (64, 5, 8),
# (64, 8, 16) and 2,048 / 8,192 / 65,536 / 262,144 rows): the kernel wins all twenty cells, the narrowest being
# (2, 8, 16) at 2,048 rows, 19.3 against 23.0 ns per row (1.19 x; at 262,144 rows 0.34 against 0.61); (64, 8, 16) at 262,144
# rows: 5.80 against 57.0.  The smallest row count from which it wins every cell is 2,048 = RT_MIN_ROWS: the value a
# follow-up that may edit the pinned test would make the default.
NSF_AR_RT_MIN_ROWS = None

# NSF_AR, the gradients of the one-pass direction (every Adam step of an NSF_AR density model) on the matrix-core kernel
# nsf_ar_bwd_rt (csrc/mnf_nsf_ar_bwd_rt.hip; flows.NSF_AR._rt_bwd): OPT-IN (RT_ROUTES "nsf_ar_bwd"; an existing
# test pins nsf_ar_bwd_generic under force_generic = 2), nsf_ar_rt's shapes with K = 5 or 8.  Under MNF_DETERMINISTIC=1 the route
# runs mnf_nsf_ar_bwd_rt_det (no atomic sums).  Measured (tools/time_nsf_ar_bwd_rt.py, profiles/r18/nsf_ar_bwd_rt_ab.txt: NSF_AR.inverse +
# backward through the layer, forward on nsf_ar_rt both times, this route against nsf_ar_bwd_generic, ns per row, at (dim, K,
# n_h) = (2, 8, 16), (6, 5, 8), (16, 8, 8), (64, 5, 8), (64, 8, 16) and 2,048 / 8,192 / 65,536 / 262,144 rows, the fixed-order form
# too at 65,536):
#   (2, 8, 16)   90.0 against 89.3 | 21.9 / 21.9 | 6.75 / 8.31 | 4.67 / 7.07 | fixed order 7.07 / 9.51
#   (6, 5, 8)    357 / 355         | 89.5 / 89.3 | 11.2 / 23.9 | 4.13 / 20.4 |             7.79 / 22.5
#   (16, 8, 8)   602 / 602         | 150 / 150   | 19.6 / 68.2 | 8.96 / 63.6 |             19.8 / 68.5
#   (64, 5, 8)   3,876 / 3,860     | 974 / 967   | 122 / 322   | 36.1 / 279  |             104 / 317
#   (64, 8, 16)  3,882 / 3,896     | 578 / 927   | 89.4 / 430  | 59.5 / 413  |             124 / 446
# At 65,536 and 262,144 rows the route wins all ten cells, the narrowest being (2, 8, 16) at 65,536 rows (6.75 against 8.31,
# 1.23 x), the widest (64, 5, 8) at 262,144 (36.1 against 279, 7.7 x), and every fixed-order cell; no cell at 65,536 rows and
# dim >= 16 is lost.  At 2,048 and 8,192 rows the step is bound by the layer's host side (packing dim - 1 nets' parameters:
# ~180 us per call at dim 2, 7.9 ms at dim 64) and the routes tie to within 1 % (six cells 0.1-0.7 % behind: noise; (64, 8, 16)
# at 8,192 rows 1.6 x ahead).  The smallest row count from which it wins every cell is 65,536: the value a follow-up that may
# edit the pinned test would make the default.
NSF_AR_BWD_RT_MIN_ROWS = None

# NSF_AR, the element-by-element direction (NSF_AR.forward: z -> x, what model.sample() of a model holding an NSF_AR runs
# through, and the density pass of an NSF_AR used the IAF way round) on the matrix-core kernel nsf_ar_seq_rt
# (csrc/mnf_nsf_ar_seq_rt.hip; flows.NSF_AR._rt_seq), forward launches only: OPT-IN (RT_ROUTES
# "nsf_ar_seq"; existing tests pin nsf_ar_generic for layer.forward under force_generic = 2 and at 4,099 rows), dim 2..128,
# K = 5 or 8, 1..4 hidden layers of widths 4..16.  Its gradients stay on nsf_ar_bwd_generic.
# Measured (tools/time_nsf_ar_seq_rt.py, profiles/r19/nsf_ar_seq_rt_ab.txt: NSF_AR.forward through the layer under no_grad,
# nsf_ar_seq_rt against nsf_ar_generic, median of 15 alternating calls, ns per row, at 2,048 / 8,192 / 65,536 / 262,144 rows):
#   (2, 8, 16)   13.5 against 22.8 | 3.28 / 5.60 | 0.422 / 0.851 | 0.166 / 0.620
#   (6, 5, 8)    28.2 / 44.0       | 6.97 / 10.9 | 0.898 / 1.76  | 0.442 / 1.27
#   (16, 8, 8)   66.9 / 119        | 16.6 / 30.9 | 2.15 / 5.30   | 1.18 / 4.54
#   (64, 5, 8)   249 / 439         | 62.3 / 113  | 8.56 / 33.7   | 5.76 / 31.9
#   (64, 8, 16)  264 / 541         | 65.9 / 145  | 9.12 / 58.8   | 6.29 / 57.0
# The kernel wins all twenty cells, each by more than the min-max spread of that cell's nsf_ar_generic timings, the narrowest
# being (6, 5, 8) at 2,048 rows (1.56 x), the widest (64, 8, 16) at 262,144 (9.06 x).  The smallest row count from which it wins
# every cell is 2,048 = RT_MIN_ROWS: the value a follow-up that may edit the pinned tests would make the default.
NSF_AR_SEQ_RT_MIN_ROWS = None

# AffineHalfFlow gradients for conditioners whose widest hidden layer has 65 .. 128 units (h_sizes = (128, 128, 128), (96,),
# ...) on the second size class of the matrix-core kernel ahf_bwd_rt (csrc/mnf_ahf_bwd_rt.hip, the mnf_affine_half_bwd_rt_wide*
# entries; flows._ahf_bwd_rt_wide): OPT-IN (RT_ROUTES "ahf_bwd_wide"; an existing test pins
# ahf_bwd_generic for h_sizes = (128,) at 4,096 rows).  Under MNF_DETERMINISTIC=1 the route runs mnf_affine_half_bwd_rt_wide_det (no atomic sums); with the owner's
# fuse_rt_training a run of such layers trains as one node on the wide stack entries.
# Measured (tools/time_ahf_bwd_rt_wide.py, profiles/r20/ahf_bwd_rt_wide_ab.txt: forward + backward through the layer, forward on
# ahf_rt both times, this route against ahf_bwd_generic, median of 15 alternating calls, ns per row, at 2,048 / 8,192 / 65,536 /
# 262,144 rows, the fixed-order form too at 65,536):
#   (64, (128,))            199 against 220 | 49.7 / 56.8 | 7.87 / 23.6 | 4.24 / 18.7 | fixed order 7.69 / 23.1
#   (64, (96, 96))          183 / 316       | 45.8 / 80.7 | 10.8 / 50.2 | 7.28 / 42.3 |             11.5 / 50.5
#   (64, (128, 128, 128))   234 / 492       | 61.6 / 224  | 34.5 / 133  | 31.6 / 131  |             37.8 / 135
#   (512, (128, 128))       376 / 779       | 104 / 508   | 38.3 / 375  | 34.1 / 365  |             37.9 / 374
# The route wins all sixteen cells and every fixed-order cell; fifteen by more than the min-max spread of that cell's
# ahf_bwd_generic timings, (64, (128,)) at 8,192 rows inside it (7.1 ahead, spread 8.1).  The smallest row count from which it
# wins every cell by more than that spread is 65,536: the value a follow-up that may edit the pinned test would make the
# default.  No cell is lost at any row count.
AHF_BWD_RT_WIDE_MIN_ROWS = None

# MNFConv2d.forward behind sample_z and the operand launch as ONE matrix-core launch (csrc/mnf_mnf_conv_fwd.hip, family
# mnf_conv_fwd; layers._MnfConvFwdFn): both convolutions on the exact-fp32 matrix instruction with the noise
# epilogue fused, instead of two MIOpen convolutions, the x * x launch and the noise launch: OPT-IN.  False: forward is the
# route it has always been, launch for launch; True sends a call there wherever mnf_mnf_conv_fwd_supported has the shape
# (n_out <= 64, n_in k^2 <= 4096), at any batch size.  Its gradients stay where they are: the noise gradient launch and
# aten's convolution_backward, twice.
# Measured (tools/time_mnf_conv_fwd.py, profiles/r21/mnf_conv_fwd_ab.txt: layer.forward, this route against the current one
# timed twice, median of 15 alternating calls, microseconds per call, at batch 128 / 1,024 / 8,192):
#   MNFConv2d(1, 20, 5) 28x28   forward, no_grad   154 against 182 / 187 | 196 / 303 / 307 | 729 / 1,573 / 1,581
#                               forward + backward 572 / 600 / 604       | 917 / 997 / 1,009 | 2,852 / 3,621 / 3,628
#   MNFConv2d(20, 50, 5) 12x12  forward, no_grad   176.4 / 173.6 / 178.1 | 233 / 286 / 287 | 943 / 1,204 / 1,214
#                               forward + backward 943 / 1,002 / 1,016   | 1,042 / 1,063 / 1,060 | 4,806 / 5,050 / 5,046
#   MNFLeNet forward, no_grad   128 rows 506 / 598 / 592 | 4,096 rows 1,252 / 1,830 / 1,830
# GPU kernels per layer forward 8 against 13.  Eleven of the twelve layer cells and both LeNet lines are won by more than the
# current route's spread (1.18-2.16 x forward, 1.02-1.27 x forward + backward, where the unchanged gradient convolutions
# dominate).  Not won: the second convolution's forward at batch 128, which lands between the current route's two medians
# (level).  The smallest batch from which the route wins every cell by more than that spread is 1,024: the threshold a
# follow-up would give the switch.
MNF_CONV_FUSED = False

# The gradients of that node on the library's own kernels (csrc/mnf_mnf_conv_bwd.hip, families mnf_conv_bwd_weight and
# mnf_conv_bwd_input; layers._MnfConvFwdFn._backward_fused): OPT-IN, read at every backward call, and only
# inside _MnfConvFwdFn.backward, that is with MNF_CONV_FUSED on.  The three weight-side gradients are one matrix-core pass
# over x (the x * x tensor disappears) plus a zeroing and a fixed-order reduction launch; grad_x is one launch with the
# 2 x epilogue inside.  Each part asks its own shape query and otherwise runs what it runs with the switch off.  No atomics:
# a backward repeats bit for bit.
# Measured (tools/time_mnf_conv_bwd.py, profiles/r27/mnf_conv_bwd_ab.txt: forward + backward through the layer, fused forward
# both times, this route against the parent route timed twice, median of 15 alternating calls, microseconds per call, at
# batch 128 / 1,024 / 8,192):
#   MNFConv2d(1, 20, 5) 28x28   905 against 962 / 962 | 553 / 748 / 745 | 2,427 / 2,826 / 2,820        (weight part only)
#   MNFConv2d(20, 50, 5) 12x12  629 / 672 / 672       | 1,260 / 957 / 959 | 7,405 / 4,872 / 4,800      (both parts)
#   MNFLeNet forward + backward 128 rows 2,259 / 2,462 / 2,480 | 4,096 rows 6,962 / 5,918 / 5,868
# Five of eight cells are won by more than the parent's spread (the first convolution everywhere, everything at batch 128);
# the second convolution from batch 1,024 on and the LeNet step at 4,096 rows are LOST: both new kernels are 1.4-2.1 x slower
# there than the aten launches they replace (profiles/r27/README.md, kernel by kernel).  No batch wins every cell, so the
# switch has no threshold to offer yet.
MNF_CONV_BWD_FUSED = False

# Seeded sampling of a model that is one run of AffineHalfFlow layers on the run-time-shaped tier (ahf_rt / ahf_stack_rt) as
# ONE launch whose first layer generates its rows (csrc/mnf_ahf_rt.hip ahf_rt_sample_kernel; flows._AffineRun._launch_sample_rt,
# DESIGN.md 3.8p), with log_q from the same launch under return_log_prob=True: from this many rows on, None = never (the
# general route: mnf_normal_rows(_sq), ahf_stack_rt, mnf_gauss_logq_sq).  Read at every call; never effective below what
# _AffineRun.rt_route accepts (RT_MIN_ROWS, or any row count when every layer has force_generic = 2).
# Measured (tools/time_sample_rt.py, profiles/r31/sample_rt_ab.txt: microseconds per call, median of 15, every column a fresh
# process, general / one launch / general / one launch): the one launch wins 20 of 24 cells and is level in one, by most
# where the call is launch-bound -- (6, (8,)) x 3 at 4,096 rows 88 -> 53 (0.60 x), (64, (24, 24)) x 3 at 4,096 rows 107 -> 69
# (0.65 x), at 2^16 138 -> 99, at 2^18 244 -> 227 (0.93 x), at 2^20 835 -> 699; x 9 layers at 4,096 rows 206 -> 157, at 2^16
# 285 -> 240, at 2^18 605 -> 598 (level), at 2^20 2,095 -> 1,964 -- and LOSES three cells at the largest sizes: (64, (24, 24))
# x 9 at 2^20 rows with log_q 2,040 -> 2,113 (1.036 x), c6's model (dim 512, 9 layers) at 2^18 rows 2,820 -> 2,880 x only
# (1.021 x) and 2,678 -> 2,924 with log_q (1.092 x); at 2^16 rows c6 wins (836 -> 793, 809 -> 775).  There the in-register
# Box-Muller of layer 0 (one or two waves per SIMD at 226-256 registers) costs more than the noise tensor's round trip
# saves, and the general route's mnf_normal_rows_sq is the faster materialiser.  The lost cells are at the top of the row
# range, so no row count exists from which every cell is won or level: the switch ships None.
RT_SAMPLE_MIN_ROWS = None

NO_FUSED_LOGPROB = False  # measurements: the log-prob epilogue stays its own launch after an affine run


def rnvp_bwd_small(rows: int, dim: int) -> bool:
    """True where the per-shape matrix-core RNVP gradient pass does not pay yet (few rows, or a narrow layer at a moderate
    batch): the run-time-shaped kernel (from RT_MIN_ROWS rows on) or the VALU kernel takes the call."""
    if rows < RNVP_BWD_MFMA_MIN_ROWS:
        return True
    if dim >= RNVP_BWD_MFMA_MIN_DIM or rows >= RNVP_BWD_MFMA_ANY_DIM_ROWS:
        return False
    return not (dim >= RNVP_BWD_MFMA_MID_DIM and rows >= RNVP_BWD_MFMA_MID_ROWS)


def glow_route(rows: int, dim: int, force_generic: int = 0, weight: bool = False) -> str:
    """Tier of Glow's x @ W (forward, inverse and grad_x alike; ``weight``: of the weight gradient x^T g).  The kernels
    are fp32, so an fp32 request changes nothing; force_generic = 1 / 2: the VALU kernels / the run-time-shaped ones at
    any row count and any dim they support, per-shape dims included."""
    from . import _lib
    lib = _lib.load()
    if force_generic == 1:
        return "valu"
    rt = bool(lib.mnf_linear_rows_rt_supported(dim))
    if force_generic == 2:
        return "rt" if rt else "valu"
    if (dim == 32) if weight else lib.mnf_linear_rows_image_floats(dim) > 0:
        return "per-shape"
    return "rt" if rt and rows >= GLOW_RT_MIN_ROWS else "valu"


# ---------------------------------------------------------------------------------------------------------------------
# The table above as a function: which TIER a call lands on ("per-shape", "rt" = run-time-shaped, "valu").  The shape
# questions go to the library's own host-side queries (no GPU needed); the row-count questions are the constants above.
# tests/test_abi_symbols.py checks it against every row of the committed coverage map (profiles/r6/coverage_map.txt):
# the table, this function and the measured map cannot drift apart unnoticed.
# ---------------------------------------------------------------------------------------------------------------------
def wants_rt(rows: int, force_generic: int = 0, fp32_request: bool = False) -> bool:
    """True where a call without a per-shape kernel goes to the run-time-shaped kernels if they have its shape (the
    gradient passes ask here; the C entry points decide it the same way for the forward kernels): from RT_MIN_ROWS rows
    on, not under an fp32 request (their arithmetic is split-f16); force_generic = 1 / 2: never / at any row count."""
    return force_generic != 1 and (force_generic == 2 or (rows >= RT_MIN_ROWS and not fp32_request))


@dataclass(frozen=True)
class RtRoute:
    """One route onto a run-time-shaped kernel that the Python layer decides (rt_route)."""
    floor: str              # name of the module constant that is its row floor (looked up at every call: tests patch it)
    query: str              # the library's shape query
    by_name: bool           # class "by name" (force_generic = 2 alone reaches it, floor None included), else "opt-in"
    fp32_vetoes_by_name: bool  # an fp32 request vetoes under force_generic = 2 too (False: force_generic = 2 overrides it)


# Every Python-decided route, one row each; rt_route below is the ONE rule that reads it -- the layers' predicates
# (flows.MAF._rt / _rt_seq / _rt_seq_bwd, flows.NSF_AR._rt / _rt_bwd / _rt_seq, flows._ahf_bwd_rt_wide) and tier() ask it.
# The two classes, for a route with row floor F (its constant) and a layer's force_generic:
#   by name:  force_generic = 1 never; 2 at ANY row count, F ignored (None too); 0 needs F set, rows >= F,
#             rows >= RT_MIN_ROWS and no fp32 request.
#   opt-in:   F None never, rows < F never -- both under force_generic = 2 too; force_generic = 1 never; 2 lifts
#             RT_MIN_ROWS only; 0 needs rows >= RT_MIN_ROWS and no fp32 request.
# The last column is what an fp32 request does under force_generic = 2 (without it the request always vetoes: the kernels'
# arithmetic is split-f16): the MAF family lets force_generic = 2 override it, the later routes do not.  The shape query is
# asked last in both classes.
RT_ROUTES = {
    #                           floor constant              shape query                              by name  fp32 vetoes
    "maf":            RtRoute("MAF_RT_MIN_ROWS",           "mnf_maf_rt_supported",                  True,    False),
    "maf_bwd":        RtRoute("MAF_RT_MIN_ROWS",           "mnf_maf_bwd_rt_supported",              True,    False),
    "maf_seq":        RtRoute("MAF_SEQ_RT_MIN_ROWS",       "mnf_maf_seq_rt_supported",              True,    False),
    "maf_seq_bwd":    RtRoute("MAF_SEQ_BWD_RT_MIN_ROWS",   "mnf_maf_seq_bwd_rt_supported",          False,   False),
    "nsf_ar":         RtRoute("NSF_AR_RT_MIN_ROWS",        "mnf_nsf_ar_rt_supported",               True,    True),
    "nsf_ar_bwd":     RtRoute("NSF_AR_BWD_RT_MIN_ROWS",    "mnf_nsf_ar_bwd_rt_supported",           False,   True),
    "nsf_ar_seq":     RtRoute("NSF_AR_SEQ_RT_MIN_ROWS",    "mnf_nsf_ar_seq_rt_supported",           False,   True),
    "ahf_bwd_wide":   RtRoute("AHF_BWD_RT_WIDE_MIN_ROWS",  "mnf_affine_half_bwd_rt_wide_supported", False,   True),
}


def rt_route(name: str, rows: int, shape_args, force_generic: int = 0, fp32_request: bool = False) -> bool:
    """Does a call of ``rows`` rows take route ``name`` of RT_ROUTES?  ``shape_args``: the arguments of its shape query."""
    from . import _lib
    route = RT_ROUTES[name]
    floor = globals()[route.floor]
    if fp32_request and route.fp32_vetoes_by_name:
        return False
    if not wants_rt(rows, force_generic, fp32_request):
        return False
    if not (route.by_name and force_generic == 2) and (floor is None or rows < floor):
        return False
    return bool(getattr(_lib.load(), route.query)(*shape_args))


def tier(kind: str, direction: str, rows: int, dim: int, hidden, K: int | None = None, scale: bool = True,
         shift: bool = True) -> str:
    """Tier of one layer call (no force_generic, no fp32 request; the same under MNF_DETERMINISTIC=1): kind "ahf" |
    "nsf" | "rnvp" | "glow" | "maf" | "maf_seq" | "nsf_ar" | "nsf_ar_seq", direction "fwd" | "bwd", hidden = the conditioner's hidden widths (NSF_CL: (n_h,) * 3;
    Glow: (); Glow "bwd" is the weight gradient's tier -- grad_x has the forward pass's; "maf": the one-pass direction of
    MAF / IAF, hidden = MADE's hidden sizes; "maf_seq": their element-by-element direction, whose "bwd" is "valu"
    unless MAF_SEQ_BWD_RT_MIN_ROWS is set; "nsf_ar": NSF_AR with K and hidden = its nets' hidden widths -- "fwd" is the
    one-pass direction NSF_AR.inverse, "valu" unless NSF_AR_RT_MIN_ROWS is set; "bwd" is its gradient pass, "valu" unless
    NSF_AR_BWD_RT_MIN_ROWS is set; "nsf_ar_seq": NSF_AR's element-by-element direction NSF_AR.forward -- "fwd" is "valu"
    unless NSF_AR_SEQ_RT_MIN_ROWS is set, "bwd" is always "valu"; "ahf" "bwd" with the widest hidden layer at 65 .. 128
    units is "valu" unless AHF_BWD_RT_WIDE_MIN_ROWS is set)."""
    from . import _lib
    if kind == "glow":
        return glow_route(rows, dim, 0, weight=direction == "bwd")
    lib, hid, n = _lib.load(), _lib.int_array(list(hidden)), len(hidden)
    if kind in ("maf", "maf_seq", "nsf_ar", "nsf_ar_seq"):  # the Python-decided routes: RT_ROUTES, one kernel or the VALU one
        if kind == "nsf_ar_seq" and direction != "fwd":  # (NSF_AR.forward's gradients have the VALU kernel only)
            return "valu"
        shape_args = (dim, n, hid) if kind.startswith("maf") else (dim, K, n, hid)
        return "rt" if rt_route(kind if direction == "fwd" else kind + "_bwd", rows, shape_args) else "valu"
    if kind == "ahf":
        if direction == "fwd":
            per_shape = lib.mnf_affine_half_image_floats(dim, n, hid, int(scale), int(shift)) > 0
        else:  # the fp32-MFMA gradient kernel's shapes contain the split kernel's
            per_shape = lib.mnf_affine_half_bwd_index_ints(dim, n, hid, int(scale), int(shift)) > 0
    elif kind == "nsf":
        tile = bool(lib.mnf_nsf_cl_bwd_tile_supported(dim, K, n, hid))
        per_shape = lib.mnf_nsf_cl_image_floats(dim, K, n, hid) > 0 if direction == "fwd" else tile
        hp = (dim // 2 + 3) // 4 * 4
        if not per_shape and hp != dim // 2 and 2 * hp <= 64 and len(set(hidden)) == 1 and rows >= NSF_PAD_MIN_ROWS:
            per_shape = bool(lib.mnf_nsf_cl_bwd_tile_supported(2 * hp, K, n, hid))  # the zero-padded twin layer
    else:
        per_shape = lib.mnf_rnvp_image_floats(dim, n, hid) > 0
        if direction == "bwd":
            per_shape = per_shape and not rnvp_bwd_small(rows, dim)
    if per_shape:
        return "per-shape"
    if not wants_rt(rows):
        return "valu"
    fwd = direction == "fwd"
    if kind == "ahf":
        query = lib.mnf_affine_half_rt_supported if fwd else lib.mnf_affine_half_bwd_rt_supported
        rt = query(dim, n, hid, int(scale), int(shift))
        if not rt and not fwd:  # (opt-in: widest 65 .. 128)
            rt = rt_route("ahf_bwd_wide", rows, (dim, n, hid, int(scale), int(shift)))
    elif kind == "nsf":
        rt = (lib.mnf_nsf_cl_rt_supported if fwd else lib.mnf_nsf_cl_bwd_rt_supported)(dim, K, n, hid)
    else:
        rt = (lib.mnf_rnvp_rt_supported if fwd else lib.mnf_rnvp_bwd_rt_supported)(dim, n, hid)
    return "rt" if rt else "valu"


def tier_of_kernel(name: str) -> str:
    """The tier a kernel family name (torch_mnf_amd.last_kernel()) belongs to."""
    return "valu" if "generic" in name else "rt" if name.endswith("_rt") or "_rt_sample" in name else "per-shape"
