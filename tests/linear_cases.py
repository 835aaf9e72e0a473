"""km_linear products (M = B, N, K) and the kernel launch_gemm runs each on, shared by tests/test_gemm_choice.py (the selection, on
the host) and tests/test_gpu_linear.py (the same products against a float64 matmul).  Not a test module.

km_gemm_kernel_choice(M, N, K, batch): 0 gemm_kernel, 1 gemm_nt_kernel<2,2,true> (64 x 64 tile), 2 <4,2,true> (128 x 64),
3 <4,4,true> (128 x 128, K <= 256), 4 <4,4,false> (128 x 128, K > 256).  The selection, from launch_gemm (km_generic.hip): with
m128 = ceil(M / 128), m64 = ceil(M / 64), n128 = ceil(N / 128), n64 = ceil(N / 64) and w4 = m128 n128, w2 = m128 n64, w22 = m64 n64,
  use4  = N > 64 and w4 >= 192;    use2 = not use4 and w2 >= 192
  gemm_nt_kernel at all only for K a multiple of 16 and M >= 64 (km_linear's operands are K-contiguous); otherwise code 0
  code 1  if neither and w22 >= 192, or if the chosen 128-row grid has fewer than 4096 workgroups
  code 3 / 4 if use4 (K <= 256 / above), code 2 if use2, code 0 otherwise."""

NAMES = ("gemm_kernel", "gemm_nt<2,2,true>", "gemm_nt<4,2,true>", "gemm_nt<4,4,true>", "gemm_nt<4,4,false>")

# (M, N, K, code): run on the GPU and checked on the host
TABLE = (
    # gemm_kernel: the eGeMAPS compression (K = 264, no multiple of 16), tiny, off-tile everywhere, M = 64 below 192 workgroups
    (1, 256, 264, 0), (3, 5, 7, 0), (65, 130, 33, 0), (64, 64, 16, 0),
    (63, 12800, 16, 0),        # 200 column tiles, but M < 64
    (896, 800, 48, 0),         # w22 = 14 x 13 = 182 < 192
    (897, 800, 40, 0),         # 195 workgroups, K % 16 = 8
    # <2,2,true>: 64 x 64 tiles
    (897, 800, 48, 1),         # w22 = 15 x 13 = 195: the first past the threshold, M = 14 x 64 + 1
    (1000, 800, 48, 1),        # M = 15 x 64 + 40, N = 12 x 64 + 32
    (3001, 1003, 16, 1),       # use4 (24 x 8 = 192 tiles of 128 x 128) below 4096: 47 x 16 tiles of 64 x 64, K = 16, N odd
    (6200, 70, 272, 1),        # w22 = 97 x 2 = 194; K above 256, N = 64 + 6, M = 96 x 64 + 56
    # <4,2,true>: 128 x 64, N <= 64 (use4 needs N > 64) and >= 4096 row tiles
    (524293, 50, 16, 2),       # 4097 row tiles, the last with 5 rows; N = 50 of 64
    # <4,4,true> / <4,4,false>: 128 x 128 and >= 4096 tiles
    (8200, 8190, 16, 3),       # 65 x 64 tiles, M = 64 x 128 + 8, N = 64 x 128 - 2, K = 16: one k step
    (8200, 8190, 272, 4),      # the same tiles, K = 17 steps
)

# (M, N, K, batch, code): the neighbours of every threshold, host only (the large ones would cost the GPU suite 300 MB each)
NEIGHBOURS = (
    (8192, 8190, 16, 1, 3), (8064, 8190, 16, 1, 1),            # 64 x 64 = 4096 tiles of 128 x 128 | 63 x 64 = 4032
    (8192, 8192, 256, 1, 3), (8192, 8192, 272, 1, 4),          # K = 256 | the next multiple of 16
    (8192, 8192, 264, 1, 0),                                   # K no multiple of 16
    (524288, 64, 16, 1, 2), (524160, 64, 16, 1, 1),            # 4096 row tiles of 128 x 64 | 4095
    (524288, 65, 16, 1, 3),                                    # N = 65: use4 with 4096 x 1 tiles
    (12224, 64, 16, 1, 0), (12225, 64, 16, 1, 1),              # w22 = 191 | 192 with w2 = 96
    (64, 12288, 16, 1, 1), (64, 12224, 16, 1, 0),              # M = 64: w22 = 192 | 191
    (63, 12288, 16, 1, 0),                                     # M = 63: gemm_nt_ok refuses
    # the batched products of the generic chain at d_model 128, window 128, 4 heads (tests/test_gpu_generic_shapes.py):
    (112, 80, 128, 47, 0), (112, 80, 128, 48, 1),              # scores: 2 x 2 x B
    (80 * 76, 128, 128, 1, 0), (80 * 77, 128, 128, 1, 1),      # value projection: ceil(80 B / 64) x 2
    (28 * 436, 64, 128, 1, 0), (28 * 437, 64, 128, 1, 1),      # decoder: ceil(28 B / 64) x 1
)
