"""The crop counts at which the keypoint CNN's launch schedule changes (csrc/net.hip: Net::plan_block, gemm_form, gemm_maybe_pooled, Net::hourglass), found by the
code: schedule_breaks scans PkpNet.schedule_bytes -- the dry run tests/test_gpu_net_schedule.py pins at 12 counts -- over every crop count up to 130 and reports
where the per-kind byte sums or the launch count stop being affine in L.  CROPS are the counts tests/test_gpu_net_boundaries.py RUNS the whole network at; its
first check holds them to the scan, so a new threshold in plan_block fails there until its counts are added here.

What each break is (product build; t = tiles of 4 x 8 pixels, T = tiles of 8 x 16 pixels of a launch; a|b = the schedule differs between a and b crops):
  f16x2   8|9     64x64 fused tails leave the eight-wave form (T = 32 L > 256) and carry the next block's conv1
          16|17   8x8 blocks per layer -> one launch (t = 2 L >= 33)
          24|25   32x32 blocks one launch -> Winograd + fused tail (t = 32 L > 768)
          32|33   4x4 blocks per layer -> one launch (t = L >= 33); 32x32 tails leave the eight-wave form (T = 8 L > 256)
          96|97   16x16 blocks one launch -> Winograd + fused tail (t = 8 L > 768)
          128|129 16x16 tails leave the eight-wave form (T = 2 L > 256)
          1|2, 4|5  NOT seen by the scan, taken from plan_block: the one-launch block moves from the fp32 kernel to the fp16 kernel at t >= 33 (32x32 from 2 crops,
                  16x16 from 5).  Both kernels are accounted the same bytes (4 per weight element) and one launch, so b(L) stays affine across the switch.  (The
                  GEMM-form switches at 4096 rows -- 32x32 at 3|4, 16x16 at 15|16 -- meet no per-layer block on this pipe: those maps run one launch there.)
  bf16x3  1|2     r1: direct conv2 -> Winograd (T >= 256 at 128x128), its GEMMs reach 32768 rows: split operands, the max-pool in conv3's epilogue (one launch
                  less); flags 2 only, 1 has no left neighbour
          4|5     32x32 one launch: fp32 kernel -> bf16x3 kernel (t = 32 L >= 129)
          7|8     64x64: per layer with direct conv2 -> Winograd + fused tail (T = 32 L >= 256), GEMMs from 32768 rows on split operands
          16|17   16x16 one launch: fp32 kernel -> bf16x3 kernel (t = 8 L >= 129)
          24|25   32x32 one launch -> per layer (t > 768, T = 8 L < 256: neither range)
          31|32   32x32 per layer -> Winograd + fused tail (T = 256; 32768 rows)
          64|65   8x8 per layer -> one launch (t = 2 L >= 129)
          96|97   16x16 one launch -> per layer
          127|128 16x16 per layer -> Winograd + fused tail
          128|129 4x4 per layer -> one launch (t = L >= 129)
  f32     1|2     r1: direct conv2 -> Winograd
          3|4     r1's conv3 + skip GEMM takes the max-pool into its epilogue from 512 output tiles of 128 x 128 (gemm_maybe_pooled): one launch less.  The issue's
                  reading of plan_block did not list it -- it is not in plan_block
          4|5, 16|17  32x32 / 16x16 one launch (fp32 kernel, t < 129) -> per layer
          7|8, 31|32, 127|128  64x64 / 32x32 / 16x16 per layer -> Winograd + fused tail
The scan reported no count that is not a schedule change: no term of the accounting is non-affine inside one schedule.  With and without priors give the same
breaks (the two staging layouts differ in their first launch only).  A default network moved to the bf16x3 form (the fp16 form's fall-back) has the breaks of
the SUO_F16X2=0 build.

NOT covered (beyond 129 crops nothing fits a test of a few seconds): 8x8 one launch -> per layer at 384|385, 4x4 at 768|769, the 2 GiB limit of gemm_bf16x3_takes
at 512 crops."""
from suo_slam_amd.pkpnet import PkpNet

PIPES = {"f32": 0, "bf16x3": 1, "f16x2": 2}
SCAN_L_MAX = 130

CROPS = {"f16x2": (1, 2, 4, 5, 8, 9, 16, 17, 24, 25, 32, 33, 96, 97, 128, 129),
         "bf16x3": (1, 2, 4, 5, 7, 8, 16, 17, 24, 25, 31, 32, 64, 65, 96, 97, 127, 128, 129),
         "f32": (1, 2, 3, 4, 5, 7, 8, 16, 17, 31, 32, 127, 128)}
# members of CROPS the scan cannot report: 1 has no left neighbour; f16x2's 1|2 and 4|5 are a change of kernel the accounting does not see (above)
UNSEEN = {"f16x2": {1, 2, 4, 5}, "bf16x3": {1}, "f32": {1}}
# the breaks tests/test_gpu_net_schedule.py's docstring names, per pipe: a scan that finds nothing, or loses one of these, fails
DOCUMENTED = {"f16x2": {8, 9, 16, 17, 32, 33}, "bf16x3": {4, 5, 7, 8, 16, 17, 31, 32, 64, 65, 127, 128, 129}, "f32": {2, 7, 8, 31, 32, 127, 128}}

# the prior-less route's input: eight boxes on one 640 x 480 frame -- the three of tests/test_gpu_cnn.py::test_forward_matches_oracle_end_to_end, one wider and one
# taller than 256 pixels (more than one sample per bin), a small one (bins smaller than a pixel), the whole frame, one leaving the image at the right and the bottom
FRAME_SEED = 21
BOXES = ((100, 80, 300, 290), (350.5, 100.25, 600, 400), (10, 200, 130, 330), (40, 30, 420, 250), (222.75, 17.5, 431.25, 303.125), (300, 200, 340, 236),
         (0, 0, 640, 480), (520, 360, 700, 540))


def schedule_vector(net, L, with_priors):
    """b(L): the six per-kind byte sums of one call of L crops on the network's current pipe, then its launch count -- integers below 2^53."""
    b = net.schedule_bytes(L, with_priors=with_priors)
    v = [b[k] for k in PkpNet.SCHEDULE_KINDS]
    assert all(x == int(x) and 0 <= x < 2.0 ** 53 for x in v), (L, v)
    return tuple(int(x) for x in v) + (int(b["launches"]),)


def schedule_breaks(net, pipe, with_priors, l_max=SCAN_L_MAX):
    """Every L in 2 ... l_max - 1 at which b(L + 1) - b(L) != b(L) - b(L - 1), compared exactly: within one schedule every term of b is affine in L, so a change of
    schedule between a and a + 1 reports both a and a + 1.  A dry run (PkpNet.schedule_bytes): nothing executes.  Leaves the network on `pipe`."""
    net.set_pipe(pipe)
    assert net.pipe() == pipe
    b = {L: schedule_vector(net, L, with_priors) for L in range(1, l_max + 1)}
    return [L for L in range(2, l_max) if any(b[L + 1][i] - b[L][i] != b[L][i] - b[L - 1][i] for i in range(len(b[L])))]
