/*
 * varsep_hip.h -- C ABI of libvarsep_hip.so: the MI355X (gfx950) kernels behind the var_sep training
 * hot path (encoders E_s/E_t -> residual latent integrator -> decoder D, forward and backward).
 *
 * The reference (JeremieDona/spatiotemporal_variable_separation) has no native layer: every numeric
 * op on this path is a stock torch.nn call that lands in ATen.  The entry
 * points below are therefore what a maintainer would bind in place of those ATen calls; each one
 * cites the reference call site(s) it replaces (paths relative to /root/reference/var_sep).
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (torch); the library never allocates,
 *     frees or keeps a pointer after the call returns; workspaces are passed in explicitly;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream)
 *     and is legal inside hipGraph stream capture (no allocation, no synchronisation);
 *   - return value: VS_OK (0) or a negative VS_ERR_* code; nothing throws; vs_last_error() returns a
 *     static description of the most recent failure on the calling thread;
 *   - matrices are row-major; tensors are NCHW contiguous unless a leading dimension is given;
 *   - dtype codes: VS_F32 = 0, VS_BF16 = 1, VS_F16 = 2.  "Compute type" selects the MFMA family: VS_F32 runs the
 *     exact-fp32 v_mfma_f32_32x32x2_f32 path (parity mode, <=1e-3 vs the fp32 CPU oracle is met with
 *     orders of magnitude to spare), VS_BF16 / VS_F16 run v_mfma_f32_32x32x16_{bf16,f16} with fp32
 *     accumulation.  Wherever a signature says VS_F32|VS_BF16 for a storage dtype, VS_F16 is accepted too.
 */
#ifndef VARSEP_HIP_H
#define VARSEP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VS_OK 0
#define VS_ERR_ARG (-1)       /* bad argument (null pointer, negative size, unsupported enum) */
#define VS_ERR_WORKSPACE (-2) /* workspace too small: call the matching *_workspace_bytes query */
#define VS_ERR_LAUNCH (-3)    /* hipLaunchKernel failed; see vs_last_error() */
#define VS_ERR_UNSUPPORTED (-4)

#define VS_F32 0
#define VS_BF16 1
#define VS_F16 2 /* IEEE half: the operand type of the reference's --torch_amp (torch.cuda.amp autocast, train.py:96-97) */

/* activation codes (networks/utils.py:50-72 activation_factory) */
#define VS_ACT_NONE 0
#define VS_ACT_RELU 1
#define VS_ACT_LEAKY 2 /* LeakyReLU(0.2) */
#define VS_ACT_SIGMOID 3
#define VS_ACT_TANH 4
#define VS_ACT_ELU 5

/* operand layouts of vs_gemm: element (i, k) of an operand with leading dimension ld lives at
 *   VS_LAYOUT_R : ptr[i * ld + k]   (reduction index k contiguous)
 *   VS_LAYOUT_S : ptr[k * ld + i]   (output index i contiguous)                                    */
#define VS_LAYOUT_R 0
#define VS_LAYOUT_S 1

const char* vs_version(void);
const char* vs_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * vs_gemm: C[m, n] = epilogue( sum_k A(m, k) * B(n, k) ),  m < M, n < N, k < K.
 *
 * Replaces the dense contractions of the path:
 *   nn.Linear forward            networks/mlp.py:40, networks/conv.py:124        A=x (R), B=W[out,in] (R)
 *   nn.Linear input gradient     (autograd of the above)                          A=dy (R), B=W (S)
 *   nn.Linear weight gradient    (autograd of the above)                          A=dy (S), B=x (S)
 *   ConvTranspose2d k4 s1 p0 on a 1x1 map (conv.py:258,295) and Conv2d k4 valid on a 4x4 map
 *   (conv.py:170), which are plain GEMMs over flattened weights.
 *
 * Epilogue, applied in this order to the fp32 accumulator v of element (m, n):
 *   v *= alpha;  v += bias[n] (if bias);  v = act(v);
 *   v *= act'(mask[m*ldmask+n]) (if mask: derivative of `mask_act` evaluated from its OUTPUT value --
 *        1/0 for ReLU, 1/0.2 for LeakyReLU, y(1-y) for sigmoid, 1-y^2 for tanh; fuses the activation
 *        backward of the previous layer into the input-gradient GEMM);
 *   v += C_old[m, n] (if accumulate);  store as c_dtype.
 *
 * compute: VS_F32 (A, B stored fp32) or VS_BF16 (A, B stored bf16).  c_dtype / mask_dtype: VS_F32|VS_BF16.
 * Any M, N, K >= 1 and any ld are accepted (unaligned shapes take a scalar load path).
 * workspace: only used when the library chooses split-K (few output tiles, long K); query
 * vs_gemm_workspace_bytes(M, N, K) for an upper bound.  May be NULL when that bound is 0.
 */
/* `batch` independent GEMMs of one shape in one launch: problem i reads A + i*stride_a, B + i*stride_b (elements of the compute
 * type; multiples of 16 bytes keep the vector loads) and writes C + i*stride_c (elements of c_dtype); no bias / activation / mask.  Used for the weight
 * gradients of the integrator's residual blocks (reference: resnet.py:22-50, three Linear layers per block).              */
size_t vs_gemm_batched_workspace_bytes(int batch, int64_t M, int64_t N, int64_t K);
int vs_gemm_batched(int compute, int batch, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, int64_t stride_a, int layout_a,
                    const void* B, int64_t ldb, int64_t stride_b, int layout_b, void* C, int64_t ldc, int64_t stride_c, int c_dtype,
                    float alpha, int accumulate, void* workspace, size_t workspace_bytes, void* stream);

size_t vs_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K);

/* Which tile kernel, in how many K splits, vs_gemm_batched (vs_gemm: batch 1, strides 0) runs for these arguments.  Host only, no GPU call;
 * A and B are looked at for alignment only.  out[12]: kind (0 register-staged tile, 1 LDS-DMA 128x128 tile, 2 128x128 ring tile, 3 256x256
 * tile, 4 staggered 256-row tile), tile rows, tile columns, splits, K tiles per split, tiles along M, tiles along N, ring stages (kind 2),
 * ni, mi (kind 4), 1 if split-K may be finished inside the launch (VS_GEMM_SPLITK_FUSED), workspace bytes this call needs.             */
int vs_gemm_plan(int compute, int batch, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, int64_t stride_a, int layout_a,
                 const void* B, int64_t ldb, int64_t stride_b, int layout_b, int64_t* out);

int vs_gemm(int compute, int64_t M, int64_t N, int64_t K,
            const void* A, int64_t lda, int layout_a,
            const void* B, int64_t ldb, int layout_b,
            void* C, int64_t ldc, int c_dtype,
            float alpha, const float* bias, int act,
            const void* mask, int64_t ldmask, int mask_dtype, int mask_act,
            int accumulate,
            void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Element-wise / reduction helpers around the GEMMs.
 */

/* dst[i] = (dst_dtype) src[i], i < n.  fp32 master weights -> bf16 shadow copies, input frames -> bf16.
 * Any element-aligned src / dst: four elements per access where both are aligned to four elements, one at a time otherwise
 * (vs_act_fwd and vs_act_bwd likewise). */
int vs_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);

/* Strided 2-D copy with conversion: dst[r*ldd + c] = src[r*lds + c], r < rows, c < cols.
 * Used to cut the encoder's temporal window out of the [B, T, C*H*W] frame tensor without a
 * host-side slice (train.py:76 full_data[:, t_random - nt_cond : t_random]); when `col_offset_dev`
 * is non-NULL the source column offset is *col_offset_dev * col_offset_scale, read on the device, so
 * a captured hipGraph stays valid when the random window moves.                                      */
int vs_copy2d(const void* src, int src_dtype, int64_t lds, void* dst, int dst_dtype, int64_t ldd,
              int64_t rows, int64_t cols, const int32_t* col_offset_dev, int64_t col_offset_scale, void* stream);
/* Two windows of one [rows, lds] source stacked into a [2 rows, ldd] operand in one launch (the E_t input [random window; conditioning
 * window] of train.py:45-88): rows [0, rows) from src + elem_offset_a + *col_offset_dev * col_offset_scale, rows [rows, 2 rows) from
 * src + elem_offset_b (offsets in elements; the device offset may be NULL).  Converts between the three element types.             */
int vs_copy2d_pair(const void* src, int src_dtype, int64_t lds, void* dst, int dst_dtype, int64_t ldd, int64_t rows, int64_t cols,
                   const int32_t* col_offset_dev, int64_t col_offset_scale, int64_t elem_offset_a, int64_t elem_offset_b, void* stream);

/* out[n] (+)= sum_m X[m*ldx + n]  (fp32 out).  Bias gradient of nn.Linear / conv (autograd of
 * mlp.py:40).  `accumulate` = 0 overwrites.  Internally zeroes/accumulates with float atomics over row
 * blocks, so results can differ in the last bits between runs (documented in DESIGN.md).            */
int vs_colsum(const void* X, int x_dtype, int64_t ldx, int64_t M, int64_t N, float* out, int accumulate,
              void* stream);

/* Up to 12 column-sum jobs in ONE launch (all bias gradients of a Linear chain or of the integrator): job j adds the
 * column sums of X[j] ([M[j], N[j]], leading dimension ldx[j]) into out[j][0..N[j]).  All arrays are HOST arrays of
 * n_jobs entries.  When zero_base is non-NULL, zero_count floats starting there are cleared first (lay the outputs out in
 * one flat buffer and clear it with this single memset).                                                               */
int vs_colsum_multi(int n_jobs, const void* const* X, const int* x_dtype, const int64_t* ldx, const int64_t* M, const int64_t* N,
                    float* const* out, float* zero_base, int64_t zero_count, void* stream);

/* Batch assembly from a simulation set resident in HBM (reference: data/wave_eq.py:67-72 `WaveEq.__getitem__` and :86-90
 * `WaveEqPartial.__getitem__`, for a whole batch of sampler indices): data [n_seq, nt, frame_elems] fp32; item b =
 * item_idx[b] selects sequence item / windows_per_seq and first frame item % windows_per_seq; out [batch, seq_len, frame_elems]
 * (or [batch, seq_len, n_pixels] when pixel_idx != NULL picks n_pixels fixed positions of every frame) in out_dtype.
 * Item indices outside [0, n_seq * windows_per_seq) are the caller's error (the sampler draws from that range).          */
int vs_gather_windows(const float* data, int64_t n_seq, int64_t nt, int64_t frame_elems, const int32_t* item_idx, int batch,
                      int windows_per_seq, int seq_len, const int32_t* pixel_idx, int n_pixels, void* out, int out_dtype,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * ConvTranspose2d k4 s2 p1 forward without any column matrix (reference: the three middle layers of DCGAN64Decoder,
 * networks/conv.py:259-262 `make_conv_block(nn.ConvTranspose2d(.., 4, 2, 1, bias=False), ..)` and their BatchNorm2d).
 * "Tap GEMM + col2im epilogue" (csrc/vs_conv_tap.hip): per block of 16 output channels and tile of 256 input pixels (whole
 * images of 4x4, 8x8 or 16x16) one 256x256 MFMA tile over K = Cin whose rows are (tap, channel); the input tile is staged in LDS
 * by LDS-DMA straight from NCHW, the 16 tap maps are combined in LDS, rounded once, written as 16-byte output runs.
 *   vs_convt_tap_supported : 1 when the geometry is served (16-bit compute, square 4x4 / 8x8 / 16x16 inputs, Cin % 8 == 0,
 *                            Cin >= 32, Cout >= 8, (B / groups) % (256 / (H*W)) == 0), else 0 -> use vs_conv_transpose2d_fwd.
 *   vs_convt_tap_pack_weight: fp32 master weight [Cin][Cout][4][4] -> dst [ceil(Cout/16)][16 taps x 16 channels][Cin] (compute type;
 *                            vs_convt_tap_packed_elems elements), once per optimizer step.
 *   vs_convt_k4s2_tap_fwd  : y [B, Cout, 2H, 2W] (compute type) = convT(x [B, Cin, H, W]) + bias.  bn_sums (fp64 [groups][Cout][2],
 *                            may be NULL): sum and sum of squares of the STORED outputs per (BatchNorm call group, channel),
 *                            zeroed and accumulated by this call -- feeds vs_bn_stats_from_sums, replacing the vs_bn_stats pass.
 *   vs_bn_stats_from_sums  : vs_bn_stats's outputs (mean, invstd [groups, C]; running statistics folded group by group) from
 *                            those sums; n_per_group = elements per (group, channel).                                        */
int vs_convt_tap_supported(int compute, int B, int Cin, int H, int W, int Cout, int groups);
size_t vs_convt_tap_packed_elems(int Cin, int Cout);
int vs_convt_tap_pack_weight(int compute, const float* w, int Cin, int Cout, void* dst, void* stream);
int vs_convt_k4s2_tap_fwd(int compute, const void* x, const void* w_tap, const float* bias, void* y, double* bn_sums, int B, int Cin, int H,
                          int W, int Cout, int groups, void* stream);
/* vs_convt_k4s2_tap_fwd with an fp32 output tensor (no BatchNorm sums): the fp32 parity mode (VARSEP_FP32_SPLIT) assembles the fp32 transposed
 * convolution -- ConvTranspose2d k4 s2 p1 forward, conv.py:260-263, and the input gradient of Conv2d k4 s2 p1, conv.py:119-122 -- from six launches
 * on bf16 pieces of its operands.                                                                                                     */
int vs_convt_k4s2_tap_fwd_f32(int compute, const void* x, const void* w_tap, const float* bias, float* y, int B, int Cin, int H, int W, int Cout,
                              void* stream);
/* Conv2d k3 s1 p1 the same way (reference: every 3x3 block of EncoderSST / DecoderSST(_Skip) conv.py:323-426, ConvResBlock
 * resnet.py:53-88, VGG64Encoder / VGG64Decoder conv.py:127-171, 267-320) on 4x4 / 8x8 / 16x16 maps: tile rows = 9 taps x 28
 * channels, out[m][y][x] = sum_t G_t[m][y+ky-1][x+kx-1] in the epilogue.  The input gradient is the same kernel on dz with the
 * weight read transposed and flipped: pack with flip = 1, Cin := the conv's Cout, Cout := the conv's Cin.
 * y_dtype may be VS_F32 (a module's final block keeps fp32 outputs).                                                        */
int vs_conv_k3_tap_supported(int compute, int B, int Cin, int H, int W, int Cout, int groups);
size_t vs_conv_k3_tap_packed_elems(int Cin, int Cout);
int vs_conv_k3_tap_pack_weight(int compute, const float* w, int Cin, int Cout, int flip, void* dst, void* stream);
int vs_conv_k3s1_tap_fwd(int compute, const void* x, const void* w_tap, const float* bias, void* y, int y_dtype, double* bn_sums, int B,
                         int Cin, int H, int W, int Cout, int groups, void* stream);
/* Conv2d k3 s1 p1 on a FEW 16x16 maps with many channels -- the ConvResnet integrator of the SST recipe (ConvResBlock resnet.py:53-70:
 * 64 -> 512 -> 512 -> 64 on 8 maps, applied once per predicted frame) -- as ONE launch that fills the chip: workgroup = (image, 32 output
 * channels, split of the input channels), the split's channels of the image in LDS, weights streamed in MFMA fragment order from the
 * pre-pack, the x shift of the taps taken on the result.  The split partial sums go to fp32 slabs
 * [vs_conv3_img16_splits(B, Cin, Cout)][B][Cout][256] WITHOUT bias; vs_bn_train_fwd_small_slabs (conv bias + BatchNorm + activation)
 * or vs_slab_sum (bias, output type) consume them.  Input gradient: the same call on dz with the weight packed with flip = 1,
 * Cin := the conv's Cout, Cout := the conv's Cin.  Cin must be a multiple of 64.                                                  */
int vs_conv3_img16_supported(int compute, int B, int Cin, int H, int W, int Cout);
int vs_conv3_img16_splits(int B, int Cin, int Cout);
size_t vs_conv3_img16_packed_elems(int Cin, int Cout);
int vs_conv3_img16_pack_weight(int compute, const float* w, int Cin, int Cout, int flip, void* dst, void* stream);
/* Up to 96 such pre-packs in ONE launch (every weight changes once per optimizer step, so all packs of a network are stale together:
 * 36-67 launches of ~5 us per TaxiBJ / SST step otherwise): job j = vs_conv3_img16_pack_weight(compute, w[j], K[j], M[j], flip[j], dst[j]).  */
int vs_conv3_img16_pack_weights(int compute, int n_jobs, const float* const* w, const int* K, const int* M, const int* flip, void* const* dst,
                                void* stream);
int vs_conv3_img16(int compute, const void* x, const void* w_packed, float* slabs, int B, int Cin, int Cout, void* stream);
/* The same contraction for MANY maps of width 16 / 32 / 64 (every 3x3 block of EncoderSST / DecoderSST(_Skip) conv.py:323-426 and of the VGG
 * encoders / decoders conv.py:127-171, 267-320 on whole batches): workgroup = 256 consecutive pixels of one map (256 / W rows) x 32 output
 * channels, the band's rows + halo of 64 channels at a time in LDS by double-buffered LDS-DMA, no column matrix.  H a multiple of 256 / W
 * (W = 8: whole 8 x 8 maps, four per workgroup), Cin a multiple of 64; weights from vs_conv3_img16_pack_weight (flip = 1 for the input gradient); y in any type, bias added.   */
int vs_conv3_band_supported(int compute, int B, int Cin, int H, int W, int Cout);
int vs_conv3_band(int compute, const void* x, const void* w_packed, const float* bias, void* y, int y_dtype, int B, int Cin, int H, int W,
                  int Cout, void* stream);
/* Weight gradient of the same convolution without a column matrix (the backward of every Conv2d(k=3, s=1, p=1) above): workgroup = (32 output
 * channels, 32 input channels, a share of the batch's row bands); dz and three column-shifted copies of the x band in LDS, nine 32x32
 * accumulators (one per tap) per wave.  Leaves vs_conv3_wgrad_band_slabs(...) fp32 partial gradients laid out [tap][Cout][Cin] (coalesced
 * stores); vs_conv3_wgrad_band_finish adds them into [Cout][Cin][3][3] (addend = the pending gradient for an accumulating call).  W in {16, 32, 64} with H a multiple of 256 / W, or 8 x 8 maps.    */
/* ... over a batch lying in npieces (<= 64) separate tensors of maps_per_piece maps each (the remembered (dz, x) pairs of a convolution applied
 * once per predicted frame): the gradient over their concatenation without building it; slabs as for B = npieces * maps_per_piece.   */
int vs_conv3_wgrad_band_pieces(int compute, int npieces, const void* const* x, const void* const* dz, int maps_per_piece, float* slabs, int Cin,
                               int H, int W, int Cout, void* stream);
int vs_conv3_wgrad_band_finish(const float* slabs, int nslabs, const float* addend, float* out, int Cout, int Cin, void* stream);
int vs_slab_sum_grouped(const float* slabs, int nslabs, int groups, float* partial, int64_t total, void* stream);   /* first pass over many slabs */
int vs_conv3_wgrad_band_supported(int compute, int B, int Cin, int H, int W, int Cout);

/* ---- 4x4 stride-2 pad-1 convolutions without a column matrix (csrc/vs_conv_k4s2.hip).  Replaces, for the DCGAN stride-2 layers, the
 * nn.Conv2d(c, 2c, 4, 2, 1) forward / weight gradient of reference networks/conv.py:119-122 and the input / weight gradient of
 * nn.ConvTranspose2d(2c, c, 4, 2, 1) of conv.py:260-263.  A stride-2 tap never mixes the parities of the input grid, so on the four
 * parity planes of the input ("space to depth": planes [B][4 C][H/2][W/2], channel = (row parity * 2 + column parity) * C + c) the 4x4
 * window is a 3x3 stride-1 pad-1 window over 4 C channels with 2x2 non-zero taps per plane, and the row-band kernels above
 * (vs_conv3_band, vs_conv3_wgrad_band) carry it.
 *   vs_space_to_depth2          x [B][C][H][W] (16-bit, H even, W a multiple of 16) -> planes
 *   vs_conv_k4s2_pack_weight    fp32 w [M][K][4][4] -> the vs_conv3_band pre-pack over 4 K plane channels (vs_conv_k4s2_packed_elems elements):
 *                               Conv2d weight [Cout][Cin][4][4] for its forward; ConvTranspose2d weight [Cin][Cout][4][4] (M = Cin, K = Cout)
 *                               for its input gradient -- the same index order, no flip
 *   vs_conv_k4s2_wgrad_finish   slabs [nslabs][9][M][4 K] of vs_conv3_wgrad_band(x = planes of the LARGE map, dz = the SMALL map with M
 *                               channels) -> dW [M][K][4][4] (+ addend): Conv2d: M = Cout, K = Cin, large = input, small = dz;
 *                               ConvTranspose2d: M = Cin, K = Cout, large = the output gradient, small = the input                      */
int vs_space_to_depth2_supported(int compute, int B, int C, int H, int W);
int vs_space_to_depth2(int compute, const void* x, void* planes, int B, int C, int H, int W, void* stream);
size_t vs_conv_k4s2_packed_elems(int K, int M);
int vs_conv_k4s2_pack_weight(int compute, const float* w, int K, int M, void* dst, void* stream);
int vs_conv_k4s2_wgrad_finish(const float* slabs, int nslabs, const float* addend, float* out, int M, int K, void* stream);
/*   vs_conv_k4s2_band           the gather on the planes [B][4 K][H][W] -> y [B][M][H][W] (+ bias), vs_conv3_band's arguments with K in place of
 *                               Cin; K a multiple of 64 (vs_conv_k4s2_skip_form): the kernel form that streams and multiplies only the 2 x 2
 *                               taps a plane sees (the pack has the matching form), otherwise the plain 3 x 3 kernel on a zero-padded pack
 *   vs_conv_k4s2_wgrad_band     slabs [vs_conv_k4s2_wgrad_band_slabs(B, K, H, W, M)][9][M][4 K] from the planes and the small map [B][M][H][W]  */
int vs_conv_k4s2_skip_form(int K);
int vs_conv_k4s2_band(int compute, const void* planes, const void* w_packed, const float* bias, void* y, int y_dtype, int B, int K, int H, int W, int M,
                      void* stream);
int vs_conv_k4s2_wgrad_band(int compute, const void* planes, const void* small_map, float* slabs, int B, int K, int H, int W, int M, void* stream);
int vs_conv_k4s2_wgrad_band_slabs(int B, int K, int H, int W, int M);    /* slabs the call above writes (round 4: not vs_conv3_wgrad_band_slabs' count) */
/* vs_conv3_band / vs_conv_k4s2_band with the BatchNorm statistics of the output taken in the epilogue (replaces the vs_bn_stats pass behind
 * conv -> BatchNorm, reference conv.py:41-60): (sum, sum of squares) of the STORED values are added to bn_sums [groups][Cout][2] (fp64),
 * group = map / (B / groups).  vs_bn_stats_from_sums_fold turns them into mean / invstd [groups][C], folds the running estimates in call order
 * and (reset != 0) leaves the sums at zero for the next step -- one launch instead of vs_bn_stats_from_sums' two. */
int vs_conv3_band_bn_supported(int compute, int B, int Cin, int H, int W, int Cout, int groups);
int vs_conv3_band_bn(int compute, const void* x, const void* w_packed, const float* bias, void* y, int y_dtype, int B, int Cin, int H, int W, int Cout,
                     double* bn_sums, int groups, void* stream);
int vs_conv_k4s2_band_bn(int compute, const void* planes, const void* w_packed, const float* bias, void* y, int y_dtype, int B, int K, int H, int W, int M,
                         double* bn_sums, int groups, void* stream);
int vs_bn_stats_from_sums_fold(double* sums, int groups, int C, int64_t n_per_group, float* mean, float* invstd, float* running_mean, float* running_var,
                               float momentum, float eps, int reset, void* stream);
/* The same statistics without atomics (round 4; replaces the vs_bn_stats pass behind conv -> BatchNorm, reference conv.py:41-60, 119-122): every
 * workgroup writes the (sum, sum of squares) of the stored values of its 32 channels to its own row of parts [vs_conv3_band_bn_parts_rows(B, H,
 * W)][Cout][2] (fp32; row = map * bands + band, the rows of a call group are consecutive); k4 != 0: x are the parity planes [B][4 K][H][W] of a
 * k4 s2 p1 convolution (Cin = 4 K, pack of vs_conv_k4s2_pack_weight).  vs_bn_stats_from_parts_fold adds the rows of every call group in a fixed
 * order (fp64) -> mean / invstd [groups][C] and (running_mean != NULL; var_scratch [groups][C] then required) folds the running estimates in call
 * order with a second small launch.  No zero fill, reproducible launch to launch. */
int vs_conv3_band_bn_parts_rows(int B, int H, int W);
int vs_conv3_band_bn_parts(int compute, const void* x, const void* w_packed, const float* bias, void* y, int y_dtype, int B, int Cin, int H, int W, int Cout,
                           float* parts, int k4, void* stream);
int vs_bn_stats_from_parts_fold(const float* parts, int rows_per_group, int groups, int C, int64_t n_per_group, float* mean, float* invstd,
                                float* var_scratch, float* running_mean, float* running_var, float momentum, float eps, void* stream);
int vs_conv3_wgrad_band_slabs(int B, int Cin, int H, int W, int Cout);
int vs_conv3_wgrad_band(int compute, const void* x, const void* dz, float* slabs, int B, int Cin, int H, int W, int Cout, void* stream);
/* Round 4: a layer of the ConvResnet integrator (reference resnet.py:53-70: Conv2d k3 s1 p1 -> BatchNorm2d (training mode) [-> LeakyReLU]; 78 block
 * calls each way per SST step) in ONE launch instead of vs_conv3_img16 + vs_bn_train_fwd_small_slabs: the other input-channel splits' partial sums
 * and the other maps' BatchNorm statistics are exchanged inside the launch through epoch-tagged 8-byte granules (the MLP integrator's mechanism),
 * so every workgroup of the launch must be resident (vs_conv3_img16_bn_supported checks: <= 256 workgroups, splits 1 / 2 / 8).
 *   ws          vs_conv3_img16_bn_workspace_bytes() bytes, zero-filled ONCE by the caller and kept (per stream); word 0 = epoch base, word 1 =
 *               sticky error flag (a partner did not answer: results invalid), the rest exchange areas
 *   call_idx    1 .. 65535, distinct for every launch on this workspace since the last vs_exchange_epoch_advance (base += 65536; recordable)
 *   _fwd        z [B][Cout][256] (16-bit pre-BatchNorm output = round16(conv + bias), bit-identical to the two-launch path), y = act(BN(z)) in
 *               y_dtype, mean / invstd [Cout], running estimates updated; skip != NULL: xnew = skip + y (fp32) and its 16-bit copy xnew16
 *   _bwd        dz = BatchNorm + activation backward of this layer applied to dy = input gradient of the FOLLOWING layer's convolution of dz_next
 *               (w_packed: that layer's weight, flip = 1; Cin = its output channels); d gamma / d beta written or ADDED (accumulate) */
size_t vs_conv3_img16_bn_workspace_bytes(void);
int vs_conv3_img16_bn_supported(int compute, int B, int Cin, int Cout);
int vs_conv3_img16_bn_form_supported(int backward, int act, int y_dtype, int compute);   /* built: fwd LeakyReLU -> 16-bit y, fwd none -> fp32 y; bwd LeakyReLU / none */
int vs_exchange_epoch_advance(void* ws, void* stream);
int vs_conv3_img16_bn_fwd(int compute, const void* x, const void* w_packed, void* ws, unsigned call_idx, const float* bias, const float* gamma,
                          const float* beta, int act, float* running_mean, float* running_var, float momentum, float eps, void* z, void* y, int y_dtype,
                          float* mean, float* invstd, const float* skip, float* xnew, void* xnew16, int B, int Cin, int Cout, void* stream);
int vs_conv3_img16_bn_bwd(int compute, const void* dz_next, const void* w_packed, void* ws, unsigned call_idx, const void* z, const float* mean,
                          const float* invstd, const float* gamma, const float* beta, int act, void* dz, float* dgamma, float* dbeta, int accumulate,
                          int B, int Cin, int Cout, void* stream);
int vs_slab_sum(const float* slabs, int nslabs, const float* bias, const float* addend, void* out, int out_dtype, int B, int C, int64_t HW,
                void* stream);
/* Round 4: vs_slab_sum with a SECOND fp32 addend (the gradient of a ConvResBlock output that reaches the block along two paths -- the next
 * block-step and the stacked codes the decoder reads, resnet.py:66-70 / model.py:76-86 -- joins the skip gradient without an add launch). */
int vs_slab_sum2(const float* slabs, int nslabs, const float* bias, const float* addend, const float* addend2, void* out, int out_dtype, int B, int C,
                 int64_t HW, void* stream);
int vs_bn_stats_from_sums(const double* sums, int groups, int C, int64_t n_per_group, float* mean, float* invstd, float* var_scratch,
                          float* running_mean, float* running_var, float momentum, float eps, void* stream);

/* ---- convolutions between a map with many channels and the image side with 1..8 (csrc/vs_conv_thin.hip).  Replaces, for the first encoder
 * layer and the last decoder layer of every convolutional family -- nn.Conv2d(nc, 64, 4, 2, 1) (reference networks/conv.py:119),
 * nn.ConvTranspose2d(64, nc, 4, 2, 1) (conv.py:264-267), nn.Conv2d(nc, 64, 3, 1, 1) (conv.py:130-133, 345-350), nn.ConvTranspose2d(64, nc, 3, 1, 1)
 * (conv.py:300-303), nn.Conv2d(64, nc, 3, 1, 1) (conv.py:420-426) -- the forward, input-gradient and weight-gradient calls whose GEMM form has a
 * dimension of 1..8.  big [B][C][H][W], thin [B][M][S H][S W], (k, S) = (3, 1) or (4, 2), pad 1; a big pixel p = (y, x) meets the thin pixels
 * S p + t - 1 = (S y + ty - 1, S x + tx - 1).  Weights are read from the caller's 16-bit tensor: element (c, m, t) at w[c w_sc + m w_sm + t'],
 * t' = t, or k^2 - 1 - t with `flip` (a stride-1 Conv2d seen from its output side).
 *   vs_conv_thin_expand   out_big[c][p] = bias[c] + sum_{m,t} thin[m][S p + t - 1] w(c, m, t)      Conv2d forward with few input channels (w_sc = M k^2,
 *                         w_sm = k^2); ConvTranspose2d input gradient with few output channels (same strides); Conv2d k3 s1 input gradient with
 *                         few output channels (w_sc = k^2, w_sm = C k^2, flip)
 *   vs_conv_thin_reduce   out_thin[m][q] = bias[m] + sum_{c,t: S p + t - 1 = q} big[c][p] w(c, m, t)  ConvTranspose2d forward with few output channels
 *                         (w_sc = M k^2, w_sm = k^2); Conv2d k3 s1 forward with few output channels (w_sc = k^2, w_sm = C k^2, flip); M <= 4 (k 3) / 2 (k 4)
 *   vs_conv_thin_wgrad    out[c o_sc + m o_sm + t'] = (addend ? addend[..] : 0) + sum_{maps,p} big[c][p] thin[m][S p + t - 1]: both weight gradients
 *                         (Conv2d few inputs: big = dz, o_sc = M k^2, o_sm = k^2; ConvTranspose2d few outputs: big = x, same strides; Conv2d k3 s1 few
 *                         outputs: big = x, thin = dz, o_sc = k^2, o_sm = C k^2, flip); fp32 partials in `ws`, summed in a fixed order
 * C a multiple of 32, W in {8, .., 128} dividing 512, H W a multiple of 512, 16-bit operands, 16-byte aligned.                            */
int vs_conv_thin_supported(int compute, int B, int C, int H, int W, int M, int k, int stride, int pad);
int vs_conv_thin_expand(int compute, const void* thin, const void* w, int64_t w_sc, int64_t w_sm, int flip, const float* bias, void* out, int out_dtype,
                        int B, int C, int H, int W, int M, int k, int stride, void* stream);
int vs_conv_thin_reduce(int compute, const void* big, const void* w, int64_t w_sc, int64_t w_sm, int flip, const float* bias, void* out, int out_dtype,
                        int B, int C, int H, int W, int M, int k, int stride, void* stream);
size_t vs_conv_thin_wgrad_workspace_bytes(int B, int C, int H, int W, int M, int k);
int vs_conv_thin_wgrad(int compute, const void* big, const void* thin, float* ws, size_t ws_bytes, const float* addend, float* out, int64_t o_sc,
                       int64_t o_sm, int flip, int B, int C, int H, int W, int M, int k, int stride, void* stream);

/* Frame metrics of the evaluation scripts (test/mnist/test.py:136-142): for every plane pair (pred, target) [planes, H, W] fp32
 * mse[plane] = mean squared error (PSNR = 10 log10(1 / mse) follows on the host as in the reference) and ssim[plane] = mean over the
 * (H - 10) x (W - 10) "valid" window positions of the SSIM index of utils/ssim.py:81-111 (11 x 11 Gaussian window of the given
 * sigma, c1 = (k1 max_val)^2, c2 = (k2 max_val)^2) -- what `_ssim_wrapper` (test/utils.py:19-24) returns per (sample, frame, channel).
 * One launch, planes up to ~80 x 80 (VS_ERR_UNSUPPORTED beyond); either output may be NULL.                                  */
int vs_frame_metrics(const float* pred, const float* target, int64_t planes, int H, int W, float max_val, float k1, float k2, float sigma,
                     float* mse, float* ssim, void* stream);

/* One batch of Moving-MNIST training sequences rendered on the device (reference: data/moving_mnist.py:112-175 `__getitem__` +
 * `_compute_trajectory`, :177-255 `_process_collision`, deterministic mode as main.py:81-82 constructs it).
 * digits [n_digits_total, digit_h, digit_w] uint8 in HBM; init [batch, num_digits, 5] int32 = (digit index, start row, start column,
 * row speed, column speed) per digit, i.e. the five np.random.randint draws of the reference in its order; out [batch, seq_len, 1,
 * frame, frame] (fp32 or a 16-bit type): digits added at their bounced positions, clipped at 255, divided by 255.
 * Trajectories are computed in IEEE double, operation for operation as the reference does in Python floats: bit-identical frames.
 * The kernel, plan and refusals of vs_moving_mnist_testset below (a workgroup takes a chunk of >= 1 frames of a video; a digit index outside
 * [0, n_digits_total) is never read: that digit is not drawn; VS_ERR_UNSUPPORTED when the digit images exceed the LDS).               */
int vs_moving_mnist_batch(const uint8_t* digits, int64_t n_digits_total, int digit_h, int digit_w, const int32_t* init, int batch,
                          int num_digits, int seq_len, int frame_size, void* out, int out_dtype, void* stream);

/* The Moving-MNIST TEST set in one launch (reference: preprocessing/mnist/make_test_set.py:58-91, which calls `_compute_trajectory` per
 * digit and composites on the host).  digits and init [n_videos, num_digits, 5] as for vs_moving_mnist_batch.  `frames` receives the RAW
 * values 0..255 (sum of the digits, min(., 255); no division): uint8 when frames_fp32 == 0, fp32 otherwise.  Frame (t, v) starts at element
 * t * frame_stride_t + v * frame_stride_v, so one entry point writes the file's time-major uint8 [T, N, 1, F, F] and the video-major fp32
 * [N, T, 1, F, F] that the evaluation keeps in HBM.  latents [seq_len, n_videos, num_digits, 4] int32 = (rounded row, rounded column, row
 * speed, column speed) after the collision step of frame t -- what `_compute_trajectory` appends; may be NULL.  Same double arithmetic as
 * vs_moving_mnist_batch: bit-identical positions.  One workgroup per video, or per (video, chunk of >= 8 frames) below 512 videos.
 * A digit index outside [0, n_digits_total) is never read: that digit is not drawn (its latents are still written).  16-byte vector stores
 * when frame_size^2 is a multiple of 16 bytes' worth of elements and the base pointer and both strides keep frame starts 16-byte aligned;
 * element by element otherwise.  VS_ERR_ARG (nothing launched) for a null digits / init / frames, a non-positive size, num_digits outside
 * 1..8, a digit larger than the frame, or strides under which frames overlap (the faster index must step over whole frames and the slower
 * one over the whole extent of the faster one); VS_ERR_UNSUPPORTED when the trajectory table of a workgroup and the digit images exceed
 * 64 KiB of LDS (the message names the sizes).                                                                                        */
int vs_moving_mnist_testset(const uint8_t* digits, int64_t n_digits_total, int digit_h, int digit_w, const int32_t* init, int n_videos,
                            int num_digits, int seq_len, int frame_size, void* frames, int frames_fp32, int64_t frame_stride_t,
                            int64_t frame_stride_v, int32_t* latents, void* stream);

/* The same RAW test-set frames from STORED positions instead of walked trajectories: the renderer of the STOCHASTIC test set
 * (smmnist_test_*.npz), whose trajectories vs_mmnist_stochastic_trajectories walks first because they consume the random stream as they go.
 * digits as above; positions [seq_len, n_videos, num_digits, 2] int32 = (row, column) of each digit's top-left corner per frame (the walk
 * kernel's `positions` [seq_len, n_traj, 2] viewed per video); digit_idx [n_videos, num_digits] int32.  frames, frames_fp32 and the two
 * strides exactly as for vs_moving_mnist_testset: raw min(sum of the digits, 255), uint8 or fp32, time- or video-major.  Same launch
 * shape (one workgroup per video, or per (video, chunk of >= 8 frames) below 512 videos; the slice of the position table and the digit
 * images in LDS) and the same compositing code and store widths as vs_moving_mnist_testset.  A digit index outside [0, n_digits_total)
 * (that digit in no frame), or a digit not wholly inside the frame at some frame (that digit in that frame), is not drawn and sets
 * *bad = 1 (bad: optional int32 word on the device, may be NULL, left alone otherwise); the launch never reads or writes out of bounds.
 * VS_ERR_ARG (nothing launched) for a null digits / positions / digit_idx / frames, a non-positive size, num_digits outside 1..8, a digit
 * larger than the frame, or strides under which frames overlap; VS_ERR_UNSUPPORTED when the position table of a workgroup and the digit
 * images exceed 64 KiB of LDS (the message names the sizes).                                                                          */
int vs_moving_mnist_testset_place(const uint8_t* digits, int64_t n_digits_total, int digit_h, int digit_w, const int32_t* positions,
                                  const int32_t* digit_idx, int n_videos, int num_digits, int seq_len, int frame_size, void* frames,
                                  int frames_fp32, int64_t frame_stride_t, int64_t frame_stride_v, int32_t* bad, void* stream);

/* One batch of 3D Chairs sequences gathered from the decoded views resident in HBM (reference: data/chairs.py:45-64 `get_sequence` +
 * `__getitem__`, for a whole batch of items).  frames [n_objects, views_per_object, H, W, C] uint8, HWC as `np.array(Image.open(f))`
 * yields; desc [rows, 2] int32 = (object, first view); out [rows, seq_len, C, H, W] (fp32 or a 16-bit type).  Frame t of a row is view
 * (first + t) % views_per_object (the reference's wrap-around, chairs.py:56-57); a value is (float)byte / 255.f, an IEEE division: the
 * bits of the reference's float64 `/ 255` rounded to float32, for all 256 bytes.  The HWC -> CHW transposition happens in the launch.
 * A descriptor whose object is outside [0, n_objects) or whose first view is outside [0, views_per_object) writes its row as zeros and
 * sets *bad = 1 (bad may be NULL); the launch never reads out of bounds.  At most 65535 rows per launch.                              */
int vs_chairs_gather(const uint8_t* frames, int64_t n_objects, int views_per_object, int H, int W, int C, const int32_t* desc, int64_t rows,
                     int seq_len, void* out, int out_dtype, int32_t* bad, void* stream);

/* One batch of windows gathered through a table from a timeline of frames resident in HBM (reference: data/taxibj.py:74-100
 * `STMatrix.create_dataset` + `TaxiBJ.__getitem__`, for a whole batch of items).  frames [n_frames, frame_elems] fp32; first [n_windows]
 * int32 = index of the frame at position 0 of each window; item_idx [rows] int32 = the windows of the batch (both tables on the device);
 * step = +1 (forward windows) or -1 (newest frame first, as the reference stores TaxiBJ).  out [rows, seq_len, frame_elems] (fp32 or a
 * 16-bit type): out[r, k, :] = frames[first[item_idx[r]] + k * step, :], the fp32 bits or their round-to-nearest-even 16-bit cast.
 * A row whose item index is outside [0, n_windows), or whose window would leave [0, n_frames) at either end, reads nothing, is written
 * as zeros and sets *bad = 1 (bad may be NULL); the launch never reads out of bounds.  At most 65535 rows per launch.              */
int vs_gather_timeline(const float* frames, int64_t n_frames, int64_t frame_elems, const int32_t* first, int64_t n_windows, int step,
                       const int32_t* item_idx, int64_t rows, int seq_len, void* out, int out_dtype, int32_t* bad, void* stream);
/* dst fp32 [N, T, inner] = (float) src uint8 [T, N, inner]: the time-major videos of a test-set file, as decoded, into the video-major fp32
 * tensor the dataset keeps (exact: every uint8 is an fp32).  VS_ERR_ARG for a null pointer, a negative size, T * N above the grid limit or
 * dst off a 16-byte boundary; an empty tensor launches nothing (csrc/vs_data.hip).                                                                         */
int vs_u8_tn_to_f32_nt(const uint8_t* src, int64_t T, int64_t N, int64_t inner, float* dst, void* stream);

/* The WaveEq data set simulated on the device (reference: preprocessing/wave/gen_wave.py:37-92 and :121-135; csrc/vs_wave_sim.hip
 * states the equations, the border rule and torchdiffeq's 3/8-rule tableau).  One workgroup integrates one sequence of frame_size x
 * frame_size fields (frame_size must be 64: the reference's source disc is fixed to that grid) over T frames: T - 1 Runge-Kutta steps.
 *   c2     [n_seq]                 fp32   c^2 of every sequence, rounded to fp32 once
 *   source [n_seq, 3 (T - 1) + 1]  fp32   s(t) at the stage times t_i, t_i + h_i / 3, t_i + 2 h_i / 3 of every step and at t_{T-1},
 *                                         tabulated by the caller in fp64 and rounded (ops.wave_source_table)
 *   h      [T - 1]                 fp32   step sizes t[i+1] - t[i] (may be NULL when T == 1)
 *   init   [n_seq, 2, 64, 64]      fp32   initial (w, w'); NULL = zeros, as the reference starts
 *   out    [n_seq, T, 64, 64]      fp32   frame i = w after i steps (frame 0 = the initial w)
 *   minmax [n_seq, 2]              fp32   minimum and maximum of w over all frames of a sequence, before normalisation (may be NULL)
 * normalise != 0 rewrites every sequence of `out` as (x - min) / (max - min) in fp32 with an IEEE division (what data/wave_eq.py does
 * to a file on the host).  init and out must be 16-byte aligned.                                                                    */
int vs_wave_simulate(int n_seq, int T, int frame_size, const float* c2, const float* source, const float* h, const float* init, float* out,
                     float* minmax, int normalise, void* stream);

/* Crop + two-pass 8-bit resampling with integer coefficient tables: the arithmetic of PIL's ImagingResample for 8 bits per channel,
 * bit for bit (reference: preprocessing/chairs/gen_chairs.py, `img.crop(box).resize(size, Image.LANCZOS)`; csrc/vs_resample.hip states
 * the arithmetic and the kernel, ops.lanczos_coeffs builds the tables).
 *   src [n, H, W, C] uint8, HWC;  out [n, out_h, out_w, C] uint8;  C in 1..4
 *   box: columns box_x0 .. box_x0 + box_w and rows box_y0 .. box_y0 + box_h of every image, inside the image
 *   kx [out_w, ksize_x] int32 coefficients with 22 fractional bits, bx [out_w, 2] int32 = (first tap, taps) relative to the box;
 *   ky [out_h, ksize_y], by [out_h, 2] likewise for the rows.  All four are device arrays.
 * Horizontal pass over the rows of the box, rounded and clipped to uint8 (kept in LDS), then the vertical pass over that intermediate:
 *   value = clamp(((1 << 21) + sum pixel * k) >> 22, 0, 255), 32-bit accumulation, arithmetic shift.
 * The kernel clamps every bound into the box and into ksize: no table contents make it read outside src.  One launch; one workgroup per
 * image and band of 16 output columns.  Returns VS_ERR_ARG (and launches nothing) for a null pointer, a non-positive size, a box outside
 * the image, ksize < 1, more workgroups than a grid holds, or a shape whose tables + staging rows + [box_h, 16, C] intermediate exceed
 * the 160 KiB of LDS (the message names the sizes).  No alignment is required of src or out.                                          */
int vs_resample_u8(const uint8_t* src, int64_t n, int H, int W, int C, int box_x0, int box_y0, int box_w, int box_h, const int32_t* kx,
                   const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y, int out_w, int out_h, uint8_t* out,
                   void* stream);

/* PNG decoding on the device (csrc/vs_png.hip; the stream logic is csrc/vs_inflate_core.h): the IDAT streams of a batch of PNG files are
 * inflated by vs_inflate_zlib, one wave per stream, and the filtered rows are turned into pixels by vs_png_unfilter.  Per-stream results
 * are STATUS words, not return values: a damaged file fails alone, the launch returns VS_OK and its neighbours are decoded.            */
#define VS_INFLATE_OK 0
#define VS_INFLATE_HEADER 1      /* not a zlib header: CM != 8, window above 32 KiB, check bits wrong, or a preset dictionary (FDICT) */
#define VS_INFLATE_BLOCK_TYPE 2  /* reserved block type 3 */
#define VS_INFLATE_STORED_LEN 3  /* LEN and NLEN of a stored block disagree */
#define VS_INFLATE_LENGTHS 4     /* code lengths: bad repeat, too many codes, over-subscribed or incomplete set, no end-of-block code */
#define VS_INFLATE_SYMBOL 5      /* bits that are no code of the table, or an invalid length / distance symbol */
#define VS_INFLATE_DISTANCE 6    /* a distance that reaches before the start of the output */
#define VS_INFLATE_INPUT 7       /* the stream ends before the data does (also: offsets outside the packed buffer) */
#define VS_INFLATE_OUT_LONG 8    /* more output than out_len (also: out_len outside 0 .. out_stride) */
#define VS_INFLATE_OUT_SHORT 9   /* the stream ends with less output than out_len */
#define VS_INFLATE_ADLER 10      /* the Adler-32 trailer does not match the bytes produced */
#define VS_PNG_BAD_FILTER 11     /* vs_png_unfilter: a row with a filter type above 4 */

/* n zlib streams (RFC 1950 framing, RFC 1951 stored / fixed / dynamic blocks in any number, lengths 3..258, distances 1..32768,
 * overlapping copies) into n output slots, byte for byte what zlib's inflate produces; trailing bytes after the Adler-32 are ignored.
 *   packed [packed_bytes] uint8: the streams back to back; stream i is bytes offsets[i] .. offsets[i + 1] (offsets int64 [n + 1]); no
 *   alignment is required of packed, of a stream's start or of out.
 *   out: slot i is the out_stride bytes from out + i * out_stride; out_len int64 [n]: the exact number of bytes stream i must produce.
 *   status int32 [n] receives a VS_INFLATE_* code, produced int64 [n] the bytes produced (on a failure: before it was met).
 * One wave per stream; the 32 KiB history is a window in LDS that is flushed to the slot in 4 KiB pieces.  The kernel terminates on any
 * input, reads nothing outside a stream's bytes and writes nothing outside its slot (csrc/vs_inflate_core.h states why).  VS_ERR_ARG (and
 * nothing launched) for a null pointer, n < 1, packed_bytes < 0, out_stride < 1 or n above the grid limit.                             */
int vs_inflate_zlib(const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets, int64_t n, const int64_t* out_len, uint8_t* out,
                    int64_t out_stride, int32_t* status, int64_t* produced, void* stream);

/* PNG row filters undone (all five types, bpp = C, the row above the first taken as zeros): raw slot i (raw + i * raw_stride) holds H rows
 * of 1 + W * C bytes, pixels is uint8 [n, H, W, C].  status int32 [n] is vs_inflate_zlib's: an image whose status is not 0 is skipped (its
 * pixels are left as they are), and an image with a filter byte above 4 gets VS_PNG_BAD_FILTER.  One workgroup per image, one wave per
 * channel, 64 rows at a time as a skewed wavefront (lane k works on row y + k, one pixel behind lane k - 1).  VS_ERR_ARG for a null
 * pointer, a non-positive size, C outside 1..4, raw_stride < H * (1 + W * C), n above the grid limit or a row of more than 65536 bytes. */
int vs_png_unfilter(const uint8_t* raw, int64_t raw_stride, int64_t n, int H, int W, int C, uint8_t* pixels, int32_t* status, void* stream);

/* DEFLATE compression on the device (csrc/vs_deflate.hip; the logic is csrc/vs_deflate_core.h): the encoder that writes .npz members from
 * arrays in HBM.  The input is cut into independent chunks; every chunk becomes one stored, fixed or dynamic block (the smallest by exact
 * bit count) with literals and distance-1 run matches, and ends with an empty stored block (00 00 FF FF on a byte boundary), so chunks
 * concatenate by bytes into a raw RFC 1951 stream WITHOUT a final block: the writer of the stream appends 03 00.  Two matchers: RUNS
 * (vs_deflate_chunks, the default) has no window search -- content without byte runs is Huffman-coded only; WINDOW
 * (vs_deflate_chunks_window, opt-in; the logic is csrc/vs_deflate_window_core.h) also matches up to 32768 bytes back, across chunk borders. */
#define VS_DEFLATE_MIN_CHUNK 1024
#define VS_DEFLATE_MAX_CHUNK 32768    /* also the default (the size against zlib by chunk length) */
#define VS_DEFLATE_SLOT_EXTRA 10      /* worst case of a chunk: its bytes + 5 of a stored block's header + 5 of the closing marker */
#define VS_DEFLATE_MAX_HISTORY 32768  /* bytes before src that vs_deflate_chunks_window may match against: DEFLATE's window */
#define VS_DEFLATE_WINDOW_GROUP_BYTES (4 * VS_DEFLATE_MAX_CHUNK)   /* workspace of one workgroup of vs_deflate_chunks_window */
/* src [n_bytes] uint8 (no alignment, any length; the last chunk is short) -> chunk c compressed into the slot slots + c * slot_stride, its
 * byte count into sizes[c] (int64 [ceil(n_bytes / chunk_bytes)]).  One wave per chunk; nothing is written past sizes[c] bytes of a slot,
 * and sizes[c] <= chunk length + VS_DEFLATE_SLOT_EXTRA.  n_bytes == 0 launches nothing.  VS_ERR_ARG (and nothing launched) for a null
 * pointer, n_bytes < 0, chunk_bytes outside VS_DEFLATE_MIN_CHUNK .. VS_DEFLATE_MAX_CHUNK, slot_stride < chunk_bytes + VS_DEFLATE_SLOT_EXTRA
 * or more chunks than a grid holds.                                                                                                    */
int vs_deflate_chunks(const uint8_t* src, int64_t n_bytes, int chunk_bytes, uint8_t* slots, int64_t slot_stride, int64_t* sizes, void* stream);
/* vs_deflate_chunks with the WINDOW matcher: a token is a literal or a match (length 3..258, distance 1..32768), the distance code is a real
 * dynamic code, and a match's source may lie before its chunk -- in earlier chunks and in the history_bytes (0 .. VS_DEFLATE_MAX_HISTORY)
 * bytes BEFORE src, which must be readable and must be what a decoder of the concatenated stream has produced before src[0] (the bytes of
 * the same array: the next slab of an array passes min(32768, its offset)).  Never before src - history_bytes, never past a chunk's end.
 * Per chunk the exact bits of the window parse compete with those of the runs parse: sizes[c] is never above vs_deflate_chunks's for the
 * same bytes, and where the runs parse wins the slot holds vs_deflate_chunks's bytes.  Same slots, sizes and bounds as vs_deflate_chunks.
 * workspace [workspace_bytes]: VS_DEFLATE_WINDOW_GROUP_BYTES per workgroup (4-byte aligned; the per-position length and distance); the grid
 * is min(chunks, workspace_bytes / VS_DEFLATE_WINDOW_GROUP_BYTES) workgroups of one wave that loop over the chunks, so the workspace is
 * bounded by the grid, not by n_bytes, and its size changes no byte of the output.  n_bytes == 0 launches nothing.  VS_ERR_ARG (and
 * nothing launched) for vs_deflate_chunks's reasons, history_bytes outside 0 .. VS_DEFLATE_MAX_HISTORY, a null or misaligned workspace or
 * workspace_bytes below one workgroup's.                                                                                              */
int vs_deflate_chunks_window(const uint8_t* src, int64_t history_bytes, int64_t n_bytes, int chunk_bytes, uint8_t* slots, int64_t slot_stride,
                             int64_t* sizes, void* workspace, int64_t workspace_bytes, void* stream);
/* The used part of every slot to its place in one buffer: dst[offsets[c] .. offsets[c] + sizes[c]) = slot c (offsets int64 [n_chunks]: the
 * exclusive prefix sum of sizes).  A chunk whose size is outside 0 .. slot_stride or whose bytes would leave dst [dst_bytes] is not copied.
 * VS_ERR_ARG for a null pointer, n_chunks < 1 or above the grid limit, slot_stride < 1 or dst_bytes < 0.                               */
int vs_deflate_pack(const uint8_t* slots, int64_t slot_stride, const int64_t* sizes, const int64_t* offsets, int64_t n_chunks, uint8_t* dst,
                    int64_t dst_bytes, void* stream);
/* CRC-32 (the zip / zlib polynomial) of src [n_bytes] in pieces: partial[p], p < ceil(n_bytes / chunk_bytes), receives the CRC of piece p
 * advanced past the bytes that follow it (a multiplication by x^(8 bytes) mod P), piece 0 also the term of the initial state, so that
 * zlib.crc32(data, init) == ~(XOR of the partials).  One wave per piece.  n_bytes == 0 launches nothing (the CRC is init).  VS_ERR_ARG for
 * a null pointer, n_bytes < 0, chunk_bytes outside 256 .. 2^24 or more pieces than a grid holds.                                         */
int vs_crc32(const uint8_t* src, int64_t n_bytes, int64_t chunk_bytes, uint32_t init, uint32_t* partial, void* stream);

/* Chunk-parallel DEFLATE decoding on the device (csrc/vs_inflate_chunks.hip; the logic is csrc/vs_inflate_chunks_core.h on top of
 * csrc/vs_inflate_core.h): the reader of the .npz members the encoder above writes.  Such a member is a raw RFC 1951 stream cut at
 * byte-aligned empty stored blocks (00 00 FF FF); the byte after a marker is a CANDIDATE start of a SEGMENT, every candidate is decoded by
 * one wave without knowing what came before it, and the host chains the segments from offset 0 by where each one ends (ops.inflate_raw).
 * A byte whose source lies before its segment is EXTERNAL: it is left as a mark and filled in chain order by vs_inflate_resolve.          */
#define VS_INFLATE_SLOT_BYTES 32768   /* = VS_DEFLATE_MAX_CHUNK: the most a segment may produce, and the least a slot holds */
#define VS_INFLATE_REPORT_WORDS 6     /* per candidate: status (VS_INFLATE_*), end, final, bytes produced, external bytes, largest reach */
#define VS_INFLATE_MAX_BATCH 2147483647ll   /* candidates or segments per launch: the grid limit */
/* Appends to cand int64 [cap], in no particular order, offset 0 and every offset p + 4 <= comp_bytes with comp[p .. p + 3] = 00 00 FF FF.
 * *count (device, zeroed by the caller) is advanced by the number found even where it exceeds cap (entries beyond cap are not written): a
 * call with cand null and cap 0 only counts.  VS_ERR_ARG (and nothing launched) for a null comp or count, a null cand with cap != 0, a
 * negative comp_bytes or cap, or more bytes than a grid covers.                                                                        */
int vs_inflate_sync_scan(const uint8_t* comp, int64_t comp_bytes, int64_t* cand, int64_t cap, int64_t* count, void* stream);
/* One wave per candidate c < n_cand (a batch: the workspace is n_cand slots, whatever the member's size): the segment of comp
 * [comp_bytes] that starts at cand[c] is decoded until an empty stored block has been consumed (end: the byte after it), a block with
 * BFINAL = 1 has ended (final = 1, end: the next byte boundary) or an error (status != 0: a VS_INFLATE_* code; VS_INFLATE_OUT_LONG for more
 * than VS_INFLATE_SLOT_BYTES of output, VS_INFLATE_INPUT for a start outside 0 .. comp_bytes or a segment not over after 65536 bytes of
 * input).  words int64 [n_cand, VS_INFLATE_REPORT_WORDS] always receives the report.  With status 0, slots + c * slot_stride receives the
 * `produced` bytes (0 where a byte is external) and, only when the segment has external bytes, marks uint16 [n_cand, VS_INFLATE_SLOT_BYTES]
 * row c receives per byte 0 or o + 1, the source being the byte o + 1 before the segment's first output byte.  Nothing else in global
 * memory is written, on any input.  VS_ERR_ARG (and nothing launched) for a null pointer, a negative size, n_cand above
 * VS_INFLATE_MAX_BATCH, slot_stride < VS_INFLATE_SLOT_BYTES or marks off a 2-byte boundary; n_cand == 0 launches nothing.            */
int vs_inflate_segments(const uint8_t* comp, int64_t comp_bytes, const int64_t* cand, int64_t n_cand, uint8_t* slots, int64_t slot_stride,
                        uint16_t* marks, int64_t* words, void* stream);
/* The mirror of vs_deflate_pack: out[offsets[c] .. offsets[c] + sizes[c]) = the first sizes[c] bytes of slot slot_index[c], c < n (int64
 * [n] each; the chain segments of a batch, offsets their prefix sum along the chain).  A segment whose slot is outside 0 .. n_slots - 1,
 * whose size is outside 0 .. VS_INFLATE_SLOT_BYTES or whose bytes would leave out [out_bytes] is not copied.  VS_ERR_ARG for a null
 * pointer, a negative size, n or n_slots above VS_INFLATE_MAX_BATCH or slot_stride < VS_INFLATE_SLOT_BYTES; n == 0 launches nothing.    */
int vs_inflate_place(const uint8_t* slots, int64_t slot_stride, int64_t n_slots, const int64_t* slot_index, const int64_t* sizes,
                     const int64_t* offsets, int64_t n, uint8_t* out, int64_t out_bytes, void* stream);
/* Fills the external bytes of the listed segments (those of a batch's chain that have any, IN CHAIN ORDER; arguments as vs_inflate_place,
 * marks as vs_inflate_segments left them): out[offsets[c] + i] = out[offsets[c] - marks[slot_index[c]][i]] for every non-zero mark not
 * above offsets[c].  ONE workgroup, one barrier per segment: a source lies before its segment, so it was placed by the launch before or
 * filled for an earlier segment.  Launch it after vs_inflate_place of the same batch, batches in chain order.  A segment outside the
 * bounds vs_inflate_place checks is passed over.  VS_ERR_ARG for a null pointer, a negative size, n or n_slots above
 * VS_INFLATE_MAX_BATCH or marks off a 2-byte boundary; n == 0 launches nothing.                                                         */
int vs_inflate_resolve(const uint16_t* marks, int64_t n_slots, const int64_t* slot_index, const int64_t* sizes, const int64_t* offsets, int64_t n,
                       uint8_t* out, int64_t out_bytes, void* stream);

/* Block-parallel DEFLATE decoding on the device (csrc/vs_inflate_blocks.hip; the logic is csrc/vs_inflate_blocks_core.h): the reader of raw
 * RFC 1951 streams WITHOUT sync markers -- what zlib and np.savez_compressed write.  Every block of such a stream is a place to start a
 * decoder: vs_inflate_block_scan finds the bit positions where a dynamic-Huffman block header reads (the CANDIDATES), vs_inflate_block_probe
 * decodes from every candidate to the next one with the window unknown (marks as above), the host chains the spans from bit 0 by where each
 * one ends (ops.inflate_blocks; a false candidate is never the end of a span of the chain, so it is decoded and ignored),
 * vs_inflate_block_windows turns the spans' last cells into the true 32 KiB before every span of the chain, and vs_inflate_block_decode decodes
 * each span of the chain again, now with its window, straight into the output.  Positions and ends are in BITS.                        */
#define VS_INFLATE_WINDOW_BYTES 32768       /* cells a probe keeps and leaves per candidate, bytes of a window */
#define VS_INFLATE_BLOCKS_MAX_IN 1048576    /* bytes of input one span may read */
#define VS_INFLATE_CAP 12                   /* status: a span is not over after VS_INFLATE_BLOCKS_MAX_IN bytes of input */
#define VS_INFLATE_DECODE_WORDS 3           /* per span of vs_inflate_block_decode: status, end, bytes produced */
/* Appends to cand int64 [cap], in no particular order, bit position 0 and every bit position of comp [comp_bytes] from which a non-final
 * dynamic block header reads that zlib could have written: BFINAL = 0, BTYPE = 2, HLIT <= 29, HDIST <= 29, a complete code-length code,
 * lengths that fill HLIT + HDIST entries exactly (repeat code 16 never first), an end-of-block code, a complete literal/length code and a
 * distance code that is complete or has at most one code of one bit.  *count (device, zeroed by the caller) is advanced by the number found
 * even where it exceeds cap (entries beyond cap are not written): a call with cand null and cap 0 only counts.  VS_ERR_ARG (and nothing
 * launched) for a null comp or count, a null cand with cap != 0, a negative comp_bytes or cap, or more bytes than a grid covers.          */
int vs_inflate_block_scan(const uint8_t* comp, int64_t comp_bytes, int64_t* cand, int64_t cap, int64_t* count, void* stream);
/* The finder of STORED blocks, opt-in (ops.inflate_block_scan(stored=True); the candidates of both scans together are the list the probe
 * gets).  Byte offset B with B + 4 <= comp_bytes is a stored boundary when LEN (little-endian 16 bits at B) and NLEN (at B + 2) satisfy
 * (LEN ^ 0xffff) == NLEN and B + 4 + LEN < comp_bytes (a non-final block is followed by another header; LEN = 0, the sync marker
 * 00 00 ff ff, counts).  For a stored boundary B and k = 0 .. 7 the bit position q = 8 * B - 3 - k is appended when q >= 0 and every bit
 * from q to 8 * B - 1 is zero (BFINAL = 0, BTYPE = 00 and the padding): zero to eight adjacent positions per boundary, about six of them
 * false by construction (decoded and ignored, as every false candidate).  Bit 0 is not added and final stored blocks are not looked for.
 * cand, cap and *count as vs_inflate_block_scan; one pass over the stream, nothing outside comp [comp_bytes] is read.  VS_ERR_ARG (and
 * nothing launched) for a null comp or count, a null cand with cap != 0, a negative comp_bytes or cap, or more bytes than a grid covers;
 * fewer than 5 bytes launch nothing.                                                                                                    */
int vs_inflate_block_scan_stored(const uint8_t* comp, int64_t comp_bytes, int64_t* cand, int64_t cap, int64_t* count, void* stream);
/* One wave per candidate c in first .. first + n - 1 of the SORTED list cand int64 [n_cand] (a batch: the workspace is n rows whatever the
 * member's size): blocks of comp [comp_bytes] are decoded from bit cand[c] until one ends at a bit position that is in the list, a block
 * with BFINAL = 1 has ended (final = 1) or an error (status != 0: a VS_INFLATE_* code; VS_INFLATE_CAP for a span not over after
 * VS_INFLATE_BLOCKS_MAX_IN bytes of input).  The output is not capped.  words int64 [n, VS_INFLATE_REPORT_WORDS] row c - first receives
 * status, end (in bits, behind the last block consumed), final, bytes produced, external bytes and the largest reach; cells uint16
 * [n, VS_INFLATE_WINDOW_BYTES] row c - first receives the LAST min(produced, VS_INFLATE_WINDOW_BYTES) cells in order, from its start: a
 * byte's value, or 0x8000 | o for a byte whose source is the byte o + 1 before the span's first output byte.  Nothing else in global memory
 * is written, on any input.  VS_ERR_ARG (and nothing launched) for a null pointer, a negative size, first + n above n_cand, n above
 * VS_INFLATE_MAX_BATCH or cells off a 2-byte boundary; n == 0 launches nothing.                                                         */
int vs_inflate_block_probe(const uint8_t* comp, int64_t comp_bytes, const int64_t* cand, int64_t n_cand, int64_t first, int64_t n, uint16_t* cells,
                           int64_t* words, void* stream);
/* ONE workgroup walks spans 0 .. n - 1 IN CHAIN ORDER: windows uint8 [n + 1, VS_INFLATE_WINDOW_BYTES], row 0 given (the window before span
 * 0: byte j is the byte VS_INFLATE_WINDOW_BYTES - j before the span's first output byte; zeros where the stream has not begun), row k + 1
 * = the window behind span k, from row k and the cells of row slot_index[k] of cells [n_slots, VS_INFLATE_WINDOW_BYTES] as
 * vs_inflate_block_probe left them for a span of produced[k] bytes: a value stays, a mark o reads byte VS_INFLATE_WINDOW_BYTES - 1 - o of
 * row k, a span shorter than the window keeps the rest of row k in front of its own bytes.  A span whose slot is outside 0 .. n_slots - 1
 * or whose size is negative passes its window on unchanged.  VS_ERR_ARG for a null pointer, a negative size, n or n_slots above
 * VS_INFLATE_MAX_BATCH, cells off a 2-byte or windows off a 16-byte boundary; n == 0 launches nothing.                                  */
int vs_inflate_block_windows(const uint16_t* cells, int64_t n_slots, const int64_t* slot_index, const int64_t* produced, int64_t n, uint8_t* windows,
                             void* stream);
/* One wave per span k < n of the chain: a plain inflate of comp [comp_bytes] from bit start_bits[k] until a block ends at or behind bit
 * end_bits[k] (or a final block ends), with the min(offsets[k], VS_INFLATE_WINDOW_BYTES) bytes before it taken from row k of windows uint8
 * [n, VS_INFLATE_WINDOW_BYTES], written to out + offsets[k] .. + sizes[k] and nowhere else (more output is VS_INFLATE_OUT_LONG, a distance
 * before the window VS_INFLATE_DISTANCE).  words int64 [n, VS_INFLATE_DECODE_WORDS] receives status, end (bits) and bytes produced, which
 * the caller compares with the probe's.  A span with a negative offset or size or with offsets[k] + sizes[k] above out_bytes writes nothing
 * and reports VS_INFLATE_OUT_LONG.  VS_ERR_ARG for a null pointer, a negative size, n above VS_INFLATE_MAX_BATCH or windows off a 16-byte
 * boundary; n == 0 launches nothing.                                                                                                   */
int vs_inflate_block_decode(const uint8_t* comp, int64_t comp_bytes, const int64_t* start_bits, const int64_t* end_bits, const int64_t* offsets,
                            const int64_t* sizes, int64_t n, const uint8_t* windows, uint8_t* out, int64_t out_bytes, int64_t* words, void* stream);

/* PNG encoding on the device (csrc/vs_png_encode.hip; the logic is csrc/vs_png_encode_core.h on top of the two DEFLATE cores): a batch of
 * images in HBM becomes one complete PNG file per image in three launches -- the forward row filters, one DEFLATE stream per image, the
 * framing -- so that only compressed bytes are copied to the host.  S = H * (1 + W * C) is the filtered size of one image.             */
/* pixels uint8 [n, H, W, C], C in 1..4 -> raw slot i (raw + i * raw_stride, raw_stride >= S): H rows of 1 + W * C bytes, the first byte of
 * a row its filter type.  mode 0..4: every row gets that type; mode 5: adaptive -- per row the type with the least sum of |residual|, each
 * residual read as a signed byte (0x80 counts 128), a tie to the lowest type.  bpp = C; the row above row 0 of EVERY image and the pixel
 * left of column 0 are zeros.  One wave per row, four bytes per lane along the row; bytes of a slot beyond S are not written.  No
 * alignment is required of pixels or raw.  VS_ERR_ARG (and nothing launched) for a null pointer, a non-positive size, C outside 1..4, mode
 * outside 0..5, raw_stride < S, a row (1 + W * C) above 65536 bytes or more rows than a grid of four-row workgroups holds.              */
int vs_png_filter(const uint8_t* pixels, int64_t n, int H, int W, int C, int mode, uint8_t* raw, int64_t raw_stride, void* stream);
/* n_streams streams of stream_bytes >= 1 bytes each, stream s at src + s * stream_stride (stream_stride >= stream_bytes; the padding is
 * never read), every one compressed INDEPENDENTLY of the others: stream s is cut into K = ceil(stream_bytes / chunk_bytes) chunks (the
 * last one short), chunk k goes to slot s * K + k (slots + (s * K + k) * slot_stride) and its byte count to sizes[s * K + k] (int64
 * [n_streams * K]).  The K chunks of one stream, concatenated and closed with 03 00, are a raw RFC 1951 stream that inflates on its own.
 * match 0: the RUNS parse of vs_deflate_chunks (workspace may be null).  match 1: the WINDOW parse of vs_deflate_chunks_window, whose
 * history for chunk k is min(32768, k * chunk_bytes): the stream's own bytes, never before its first byte; workspace as there
 * (VS_DEFLATE_WINDOW_GROUP_BYTES per workgroup, 4-byte aligned, the grid bounded by it; its size changes no output byte).  Per stream the
 * bytes are those of vs_deflate_chunks / vs_deflate_chunks_window (history 0) on that stream alone.  VS_ERR_ARG (and nothing launched)
 * for a null pointer, a non-positive size, stream_stride < stream_bytes, match outside 0..1, chunk_bytes outside VS_DEFLATE_MIN_CHUNK ..
 * VS_DEFLATE_MAX_CHUNK, slot_stride < chunk_bytes + VS_DEFLATE_SLOT_EXTRA, more chunks than a grid holds or, with match 1, a null,
 * misaligned or too small workspace.                                                                                                  */
int vs_deflate_streams(const uint8_t* src, int64_t n_streams, int64_t stream_bytes, int64_t stream_stride, int chunk_bytes, int match,
                       uint8_t* slots, int64_t slot_stride, int64_t* sizes, void* workspace, int64_t workspace_bytes, void* stream);
/* One complete PNG file per image into files + i * file_stride: the 8-byte signature, IHDR (bit depth 8, colour type 0 / 4 / 2 / 6 for
 * C = 1 / 2 / 3 / 4, no interlace), ONE IDAT chunk (78 9C, the chunks_per_image slots of image i back to back -- slots and sizes as
 * vs_deflate_streams left them --, 03 00, the Adler-32 of the S filtered bytes at raw + i * raw_stride, big-endian) and IEND;
 * file_bytes[i] (int64 [n]) = 57 + 8 + the sum of the image's sizes.  A size outside 0 .. slot_stride (or a sum that would leave the
 * file's stride) sets file_bytes[i] = -1 and writes nothing for that image; nothing is ever written past file_stride.  One workgroup per
 * image.  VS_ERR_ARG (and nothing launched) for a null pointer, a non-positive size, C outside 1..4, raw_stride < S, chunks_per_image
 * above S, file_stride < 57 + 8 + S + VS_DEFLATE_SLOT_EXTRA * chunks_per_image, an IDAT body that could reach 2^31 bytes, or n above the
 * grid limit.                                                                                                                         */
int vs_png_assemble(const uint8_t* raw, int64_t raw_stride, const uint8_t* slots, int64_t slot_stride, const int64_t* sizes, int64_t n, int H,
                    int W, int C, int64_t chunks_per_image, uint8_t* files, int64_t file_stride, int64_t* file_bytes, void* stream);

/* NumPy's legacy random stream on the device (csrc/vs_mt19937.hip; the logic is csrc/vs_mt19937_core.h): np.random.RandomState is MT19937,
 * and its scalar randint(low, high) is masked rejection on the 32-bit outputs.  The Moving-MNIST training loader draws its table of five
 * integers per digit from a state that lives in HBM, in the order and with the values of the host loop it replaces.                     */
#define VS_MT19937_STATE_WORDS 625    /* key[624], pos */
#define VS_MT19937_MAX_COLS 8
#define VS_MT19937_MAX_ROWS (1ll << 40)
/* state uint32 [625] in HBM = key[624], pos (0 .. 624), advanced in place; lows / highs: HOST arrays of k columns, 1 <= k <= 8; out int32
 * [n_rows, k]: out[r, j] is the (r * k + j)-th scalar randint(lows[j], highs[j]) of the stream, any int32 low < high (the widest, (-2^31,
 * 2^31 - 1), included).  A column with high == low + 1 is filled with low and consumes nothing; if every column is such, the state is not
 * touched.  pos after the call is one past the output that completed the last draw; a block is regenerated only when one of its outputs is
 * needed.  One launch is ONE workgroup: a stream is one sequence, and launches on one HIP stream continue it in their order.  bad: optional
 * int32 word on the device (may be NULL), left alone on success; the kernel sets it to 1 for a pos above 624 read from the state (out and
 * the state are then untouched) and to 2 if it gave up after 64 outputs per draw plus 4096 (a state that is no stream; the state is not
 * advanced).  n_rows == 0 launches nothing.  VS_ERR_ARG (and nothing launched) for a null state / lows / highs / out, k outside 1 .. 8,
 * n_rows < 0 or above VS_MT19937_MAX_ROWS, or lows[j] >= highs[j].                                                                       */
int vs_mt19937_randint(uint32_t* state, const int32_t* lows, const int32_t* highs, int k, int64_t n_rows, int32_t* out, int32_t* bad,
                       void* stream);

/* The STOCHASTIC Moving-MNIST trajectories on the device (csrc/vs_mmnist_walk.hip; the logic is csrc/vs_mmnist_walk_core.h): the reference's
 * sampler with deterministic=False redraws the speed vector from the NumPy stream at every bounce (data/moving_mnist.py:232-234), so the
 * outputs a trajectory takes depend on the trajectory.  One launch (ONE workgroup) walks n_traj trajectories from the state in HBM, one
 * after the other in the stream's order, bit for bit the reference's values: per trajectory n_pre scalar draws randint(lows[j], highs[j])
 * (HOST arrays; training: digit index, start row, start column, row speed, column speed; n_pre == 4: the last four alone), then seq_len
 * steps of collision pass (speeds redrawn in [-max_speed, max_speed]), record, move.  With n_pre < 4 the start state of trajectory i is
 * start[i] = (row, column, row speed, column speed) of a device table int32 [n_traj, 4] and the prefix is only drawn and recorded.
 * x_max / y_max: frame - digit height / width.  Outputs (device): pre int32 [n_traj, n_pre]; positions int32 [seq_len, n_traj, 2], which
 * vs_moving_mnist_place reads as [T, n_seq, nd, 2]; latents int32 [seq_len, n_traj, 4] = (row, column, row speed, column speed), optional;
 * desc int32 [n_traj / desc_nd, 1 + desc_nd] = (video index, the digit indices pre[.., 0] of its trajectories), optional, n_pre == 5 only.
 * state as for vs_mt19937_randint: advanced past the last output consumed, a block regenerated only when an output of it is needed.
 * bad: optional device word, left alone on success; 1: pos above 624 (nothing written); 2: a draw rejected 4096 outputs in a row; 3: a
 * collision pass count above 64 -- for 2 and 3 the outputs are partly written; on every one the state is not advanced.  n_traj == 0
 * launches nothing.  VS_ERR_ARG (and nothing launched) for a null state / positions / needed table, n_pre outside 0 .. 5, seq_len < 1,
 * n_traj < 0 or above VS_MMNIST_WALK_MAX_TRAJ, x_max or y_max < 1, max_speed < 0, lows[j] >= highs[j], or a desc without its conditions. */
#define VS_MMNIST_WALK_MAX_PRE 5
#define VS_MMNIST_WALK_MAX_TRAJ (1ll << 24)
#define VS_MMNIST_WALK_STATUS_BOUNCE 3
int vs_mmnist_stochastic_trajectories(uint32_t* state, const int32_t* lows, const int32_t* highs, int n_pre, int64_t n_traj, int seq_len,
                                      int x_max, int y_max, int max_speed, const int32_t* start, int32_t* pre, int32_t* positions,
                                      int32_t* latents, int32_t* desc, int desc_nd, int32_t* bad, void* stream);

/* Evaluation scripts (test/mnist/test.py, test/mnist/test_disentanglement.py, csrc/vs_eval.hip; vs_moving_mnist_place: csrc/vs_data.hip).
 * vs_moving_mnist_place: videos composited from digits at STORED positions (test_disentanglement.py:66-86 `SwapDataset`).
 * digits [n_digits_total, digit_h, digit_w] uint8; positions [>= seq_len, n_seq, num_digits, 2] int32 = (row, column) of each object's
 * top-left corner per frame (the (sx, sy) of the test file's `latents`); desc [n_videos, 1 + num_digits] int32 = (sequence, digit index of
 * object 0 .. num_digits-1).  out [n_videos, seq_len, 1, frame, frame] (fp32 or a 16-bit type): sum of the digits, min(., 255) / 255, the
 * arithmetic, kernel and plan of vs_moving_mnist_batch.  A sequence / digit index out of range or a digit not wholly inside the frame is not drawn and sets
 * *bad = 1 (bad may be NULL); the launch never reads or writes out of bounds.                                                          */
int vs_moving_mnist_place(const uint8_t* digits, int64_t n_digits_total, int digit_h, int digit_w, const int32_t* positions, int n_seq,
                          int num_digits, const int32_t* desc, int n_videos, int seq_len, int frame_size, void* out, int out_dtype,
                          int32_t* bad, void* stream);
/* vs_frame_metrics of one prediction against n_targets candidates: pred [batch, planes_per_sample, H, W] fp32, targets [batch, n_targets,
 * planes_per_sample, H, W] fp32 -> mse / ssim [batch, n_targets, planes_per_sample] (either may be NULL).  Same window, constants and
 * operation order as vs_frame_metrics; each prediction plane is staged in LDS once for all its targets.  Planes up to ~80 x 80.      */
int vs_frame_metrics_multi(const float* pred, const float* targets, int64_t batch, int n_targets, int64_t planes_per_sample, int H, int W,
                           float max_val, float k1, float k2, float sigma, float* mse, float* ssim, void* stream);
/* x [n, channels, hw] (fp32 or a 16-bit type, widened to fp32) -> out [n, hw, channels] uint8 = (uint8)(x * 255.f): one fp32 multiply,
 * truncation toward zero (torch's `x.mul(255).byte()` for x in [0, 1]); values outside [0, 255] after the multiply saturate, NaN -> 0. */
int vs_frames_to_u8_nhwc(const void* x, int x_dtype, int64_t n, int channels, int64_t hw, uint8_t* out, void* stream);
/* The metrics of the SST evaluation script (test/sst/test.py:57-71).  pred, target [rows, T, H, W] fp32 are the NORMALISED forecasts and
 * targets of `rows` windows; consts [n_days, 4] fp32 = (mu_norm, std_norm, mu_clim, std_clim) per day; day0 [rows] int32 = the day of each
 * window's first target frame; zone [rows] int32 indexes zone_range [n_zones, 2] fp32 = (min, max).  The script multiplies [10, 1, 1]
 * per-day constants into [1, 10, 1, H, W] frames, so every frame t meets the constants of every day c = day0 .. day0 + T - 1:
 *   x'(t, c) = (x(t) * std_norm[c] + mu_norm[c]) * std_clim[c] + mu_clim[c]
 *   mse [rows, T]:     mse[r, t]     = mean over c, H, W of (pred' - target')^2
 *   ssim [rows, T, T]: ssim[r, t, c] = mean SSIM (11 x 11 Gaussian of `sigma`, valid windows, c1 = k1^2, c2 = k2^2: max_val 1) of
 *                                      (x' - min) / (max - min); the diagonal ssim[r, t, t] pairs each frame with its own day.
 * One workgroup per (row, t), one filter pass; either output may be NULL.  A row with day0 < 0, day0 + T > n_days or a zone outside
 * [0, n_zones) reads no constants, writes zeros and sets *bad = 1 (bad may be NULL).  T <= 16; planes from 11 x 11 up to ~80 x 80
 * (VS_ERR_UNSUPPORTED beyond).                                                                                                          */
int vs_sst_frame_metrics(const float* pred, const float* target, int64_t rows, int T, int H, int W, const float* consts, int64_t n_days,
                         const int32_t* day0, const int32_t* zone, const float* zone_range, int64_t n_zones, float k1, float k2, float sigma,
                         float* mse, float* ssim, int32_t* bad, void* stream);

/* Decoder input of the auto-encoding pair and of every rollout step in one launch (mlp_encdec.py:43-48 mixing applied at
 * model.py:74-83): z [B, 1+n, Cz] = mix(s [B, Cs], [t_rand [B, Ct] ; t_codes [B, n, Ct]]), mixing 0 = concat (Cz = Cs + Ct),
 * 1 = mul (Cz = Cs = Ct); out fp32, out_bf16 (may be NULL) the same values rounded for the decoder's first bf16 GEMM.
 * bwd: dz [B, 1+n, Cz] fp32 -> ds [B, Cs] (summed over the frames), dt_rand [B, Ct], dt_codes [B, n, Ct].                   */
int vs_mix_codes_fwd(const float* s, const float* t_rand, const float* t_codes, int64_t B, int n, int Cs, int Ct, int mixing, float* out,
                     void* out_lowp, int lowp_dtype, void* stream);
int vs_mix_codes_bwd(const float* dz, const float* s, const float* t_rand, const float* t_codes, int64_t B, int n, int Cs, int Ct,
                     int mixing, float* ds, float* dt_rand, float* dt_codes, void* stream);

/* All four training losses and their weighted sum in one pass (train.py:117-149, MLP-family layout):
 *   total = l_ae mse(frames[:,0], full[:,idx[0]]) + l_s mean((s_old-s_new)^2) + l_pred mse(frames[:,1:], full[:,idx[1:]])
 *           + l_t t_reg,   t_reg = 0.5 mean_b sum_c t0^2 (average_tloss: 0.5 mean_{b,c} t0^2);  lambdas = {l_ae, l_s, l_t, l_pred}
 *   (host).  n_s = number of spatial-code elements (0: no spatial term, s_old/s_new may be NULL).  Target frames: idx [G] on the
 *   device, or idx = NULL and frame 0 <-> full[:, t_random_dev[0] - ae_shift], frame g <-> full[:, first_forecast + g - 1] (the
 *   random window end of train.py:72-75 read on the device: no index tensor to build per step).
 *   fwd: out [10] floats on the device: [4] total, [5] ae, [6] zero-order, [7] pred, [8] t_reg ([0..3], [9] scratch).
 *   bwd: grad_total = upstream gradient of `total` (1 float ON THE DEVICE); writes dframes [B,G,D], ds_old, ds_new [n_s], dt0.  */
int vs_train_losses_fwd(const float* frames, const float* full, const int32_t* idx, const int32_t* t_random_dev, int ae_shift,
                        int first_forecast, int64_t B, int G, int T, int64_t D,
                        const float* s_old, const float* s_new, int64_t n_s, const float* t0, int64_t Bt, int64_t Ct,
                        int average_tloss, const float* lambdas, float* out, void* stream);
int vs_train_losses_bwd(const float* frames, const float* full, const int32_t* idx, const int32_t* t_random_dev, int ae_shift,
                        int first_forecast, int64_t B, int G, int T, int64_t D,
                        const float* s_old, const float* s_new, int64_t n_s, const float* t0, int64_t Bt, int64_t Ct,
                        int average_tloss, const float* lambdas, const float* grad_total, float* dframes, float* ds_old,
                        float* ds_new, float* dt0, int frames_act, void* dz, int dz_dtype, void* stream);
/* Both of the above in ONE pass over the frames, for an upstream gradient known when the forward runs (a recorded training step
 * passes its resident 1.0 or loss scale: `grad_total`, one float on the device): `out` as vs_train_losses_fwd; dz (the gradient of
 * the producing chain's pre-activation, compute dtype) / ds_old / ds_new / dt0 as vs_train_losses_bwd writes them.  D % 4 == 0.
 * `out` must hold 16 + 2 * 4096 floats here: the frame sums go through per-workgroup partials (no float atomics: reproducible). */
int vs_train_losses_fwd_grad(const float* frames, const float* full, const int32_t* idx, const int32_t* t_random_dev, int ae_shift,
                             int first_forecast, int64_t B, int G, int T, int64_t D, const float* s_old, const float* s_new, int64_t n_s,
                             const float* t0, int64_t Bt, int64_t Ct, int average_tloss, const float* lambdas, float* out,
                             const float* grad_total, float* ds_old, float* ds_new, float* dt0, int frames_act, void* dz, int dz_dtype,
                             void* stream);

/* The decoder's last Linear layer with the frame losses in its epilogue -- replaces, in the recorded MLP-family step, the pair
 * [last vs_gemm of MLPDecoder.forward (networks/mlp_encdec.py:43-50) ; vs_train_losses_fwd_grad (train.py:85-86, 117-149)]:
 *   frames[r = (b, g), :] = act(A[r, :] W^T + bias) is compared with full[b, target(g), :] while in registers and never stored;
 *   dz [M, N] (dz_dtype) = grad_total * k_g * (frames - target) * act'(frames), ds_old / ds_new / dt0 and out[0..8] as
 *   vs_train_losses_fwd_grad (out holds 16 + 2 * 4096 floats; the frame sums are added from one pair per workgroup, in order).
 * A [M = B * G, K] and W [N, K] 16-bit row-major (K contiguous), bias fp32 [N] or NULL, N % 4 == 0, target frames resolved on the
 * device from t_random_dev (frame 0 <-> t - ae_shift, frame g <-> first_forecast + g - 1).  VS_ERR_UNSUPPORTED when the problem does
 * not run on the 256 x 256 tile kernel: store the frames with vs_gemm and call vs_train_losses_fwd_grad.                          */
int vs_gemm_frame_loss(int compute, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* W, int64_t ldw,
                       const float* bias, int act, const float* full, const int32_t* t_random_dev, int ae_shift, int first_forecast,
                       int G, int T, const float* s_old, const float* s_new, int64_t n_s, const float* t0, int64_t Bt, int64_t Ct,
                       int average_tloss, const float* lambdas, const float* grad_total, void* dz, int dz_dtype, float* ds_old,
                       float* ds_new, float* dt0, float* out, void* stream);

/* Adam update of up to 64 fp32 tensors in one launch (reference: train.py:156-158 `optimizer.step()` on
 * torch.optim.Adam(lr, betas): weight_decay 0, amsgrad off; same operation order as torch's single-tensor path:
 *   m += (1-b1)(g-m); v = b2 v + (1-b2) g g; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps),  t = step[0] + 1).
 * `step` is an int32 ON THE DEVICE (capturable into a hipGraph); it is NOT modified here -- several vs_adam_multi calls
 * of one optimizer step (more than 64 tensors) share it, then vs_adam_step_increment bumps it once.
 * skipped (host array or NULL): optimizer steps a tensor sat out without gradient -- torch counts steps per parameter, so
 * its t is step[0] + 1 - skipped[i].
 * shadow_bf16 (array or NULL, entries may be NULL): bf16 copy of the updated parameter written in the same pass (the
 * operand copy the bf16 forward pass reads).  Tensors contiguous; 16-byte aligned ones take the vector path.
 * grad_dtype (host array or NULL = all fp32): VS_BF16 entries read their gradient as bf16 -- the data-parallel wire image of a
 * weight gradient, consumed without a cast back to fp32.                                                                  */
int vs_adam_multi(int n_tensors, float* const* params, const void* const* grads, const int32_t* grad_dtype, float* const* exp_avg,
                  float* const* exp_avg_sq, void* const* shadow_bf16, const int64_t* numel, const int32_t* skipped, int32_t* step,
                  double lr, double beta1, double beta2, double eps, void* stream);
int vs_adam_step_increment(int32_t* step, void* stream);

/* fp16 training with dynamic loss scaling (reference: train.py:96-97 `scaler = torch.cuda.amp.GradScaler()`, train.py:151-155
 * `scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()` under --torch_amp), kept on the device so that the
 * whole step stays recordable into a hipGraph.  `scale_state` is 4 fp32 words on the device:
 *   [0] loss scale S, [1] found_inf of the current step, [2] growth tracker (clean steps since the last change), [3] steps skipped.
 * vs_check_finite_multi : found_inf[0] = 1 if any element of any listed gradient (fp32 or 16-bit) is inf / NaN   (GradScaler.unscale_'s check)
 * vs_adam_multi_scaled  : vs_adam_multi with gradients read as g / S and the whole update suppressed when found_inf is set;
 *                         shadow copies are written as `shadow_dtype` (VS_BF16 | VS_F16).  scale_state NULL = plain vs_adam_multi.
 * vs_adam_step_increment_scaled : the step count does not advance on a skipped step.
 * vs_loss_scale_update  : GradScaler.update(): S *= backoff and tracker = 0 on overflow, else tracker += 1 and S *= growth every
 *                         `growth_interval` clean steps -- only while the grown S is finite (the tracker restarts either way);
 *                         clears found_inf.                                                                                       */
int vs_check_finite_multi(int n_tensors, const void* const* grads, const int32_t* grad_dtype, const int64_t* numel, float* found_inf,
                          void* stream);
int vs_adam_multi_scaled(int n_tensors, float* const* params, const void* const* grads, const int32_t* grad_dtype, float* const* exp_avg,
                         float* const* exp_avg_sq, void* const* shadow, int shadow_dtype, const int64_t* numel, const int32_t* skipped,
                         int32_t* step, double lr, double beta1, double beta2, double eps, const float* scale_state, void* stream);
int vs_adam_step_increment_scaled(int32_t* step, const float* scale_state, void* stream);
/* Caps the grid of the following vs_adam_multi* launches of this process at `blocks` workgroups (0: the default, 4096), returns
 * the previous cap.  A bucket updated WHILE backward is still running is launched with a small grid (2 workgroups per CU) so
 * that it streams HBM in the background and leaves the wave slots to the GEMMs on the critical path.                         */
int vs_adam_set_max_blocks(int blocks);
/* Weight gradient + Adam in one launch (replaces, for one 2-D parameter, the weight-gradient vs_gemm of a Linear layer -- reference
 * mlp.py:66-75 backward -- followed by its share of optimizer.step(), train.py:156-158):  G = alpha * A * B^T with the operand
 * conventions of vs_gemm is the gradient of the contiguous fp32 parameter `param` [M, N]; the epilogue updates param / exp_avg /
 * exp_avg_sq exactly as vs_adam_multi would from a stored G (`step` = the group's device step count BEFORE the increment,
 * `skipped` as there) and rewrites the 16-bit operand copy `shadow` (NULL: none).  G is never stored.  16-bit compute types;
 * operands must fit the LDS-DMA loader (16-byte aligned, leading dimensions / extents multiples of 8): VS_ERR_UNSUPPORTED
 * otherwise and nothing is launched.                                                                                          */
int vs_gemm_adam(int compute, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, int layout_a, const void* B, int64_t ldb,
                 int layout_b, float alpha, float* param, float* exp_avg, float* exp_avg_sq, void* shadow, int shadow_dtype,
                 const int32_t* step, int32_t skipped, double lr, double beta1, double beta2, double eps, void* stream);
/* vs_gemm_adam as a launch that does NOT fill the chip, for running beside a latency-bound kernel: same operands, same arithmetic, bit
 * for bit the same result; `ldp` is the leading dimension of param / exp_avg / exp_avg_sq / shadow (>= N, a multiple of 4; those
 * pointers 16-byte, shadow 8-byte aligned, VS_ERR_UNSUPPORTED otherwise).
 *   max_workgroups    the grid is at most this many workgroups, each of which walks the 128 x 128 tiles t = b, b + grid, ... in the
 *                     XCD-aware tile order; each holds all 160 KiB of a CU's LDS, so it shares a CU with no kernel that uses LDS
 *   pieces_in_flight  1, 2 or 4 row pieces of optimizer state requested ahead of the update (vs_gemm_adam: 4)
 *   cache_policy      0 plain, 1 non-temporal loads and stores of param, exp_avg, exp_avg_sq and shadow
 * The exchange guard is read ONCE per workgroup, before its first tile.  An exchange that times out in a kernel running BESIDE this
 * launch therefore does not stop it, and one that times out just before it stops some workgroups and not others: the parameter of
 * that one step may be updated in some tiles and not in others (vs_gemm_adam: the whole tensor or nothing).  Later steps are skipped
 * as a whole either way.                                                                                                        */
int vs_gemm_adam_paced(int compute, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, int layout_a, const void* B, int64_t ldb,
                       int layout_b, float alpha, float* param, float* exp_avg, float* exp_avg_sq, void* shadow, int64_t ldp,
                       int shadow_dtype, const int32_t* step, int32_t skipped, double lr, double beta1, double beta2, double eps,
                       int max_workgroups, int pieces_in_flight, int cache_policy, void* stream);
int vs_loss_scale_update(float* scale_state, float growth_factor, float backoff_factor, int growth_interval, void* stream);

/* Fused frame losses (train.py:85-86 ae_loss MSE and train.py:139 forecast MSE in one pass over the decoded frames).
 * frames [B, G, D] fp32: per sample the auto-encoding reconstruction (g = 0) followed by the G-1 forecasts; full [B, T, D]
 * fp32: every observed frame; idx [G] int32 ON THE DEVICE: frame g is compared with full[:, idx[g]].
 *   fwd: sums[0] = sum of squared errors of frame 0, sums[1] = of frames 1..G-1 (float atomics: last-bit nondeterminism).
 *   bwd: dframes[b, g, :] = coef[g == 0 ? 0 : 1] * (frames - target); coef [2] on the device = 2/N_k times the upstream
 *        gradient of loss k, so no host synchronisation is needed.  D must make rows 16-byte aligned for speed: with
 *        D % 4 != 0, or frames / full / dframes off 16-byte alignment, every element is read and written on its own.     */
int vs_frames_sse_fwd(const float* frames, const float* full, const int32_t* idx, int64_t B, int G, int T, int64_t D, float* sums,
                      void* stream);
int vs_frames_sse_bwd(const float* frames, const float* full, const int32_t* idx, int64_t B, int G, int T, int64_t D, const float* coef,
                      float* dframes, void* stream);

/* Round 4: the conv families' code losses and the weighted total in one pass (reference train.py:38-42 zero_order_loss -- with skip connections
 * over the code and every skip tensor --, :141-149 t_reg and total): pairs (a[j], b[j]) of count[j] elements (a multiple of 8, 16-byte aligned,
 * fp32 or 16-bit: read where they lie, no concatenation), t0 [t_count] fp32, the raw sums of vs_frames_sse_fwd for the two frame terms.
 *   _fwd   out[0..4] = total, ae, zero, pred, t_reg; partial: vs_code_losses_chunks() floats (per-chunk sums, finished in a fixed order)
 *   _bwd   for the upstream gradient g[0] (device): da[j] / db[j] (NULL: not wanted) in dtype[j], dt0, and coefs[4] = the coefficient pairs
 *          vs_frames_sse_bwd takes for the auto-encoding and the forecast frame stacks.  One launch. */
/* Round 4: decoder inputs of a batched rollout (reference conv.py:228, 388-394: torch.cat([skip, out], 1) with the skip / spatial code of the B
 * sequences shared by the n frame calls that run as one batch): out [n B][Ca + Cb][HW] = cat(a [B][Ca][HW] repeated over the frames, x [n B][Cb][HW])
 * in out's type, one pass (no repeated copy of a); _bwd: da = sum over the frames of dout's first Ca channels (frame order), dx = the others.
 * HW a multiple of 8, tensors 16-byte aligned; da or dx may be NULL. */
int vs_cat_bcast_fwd(const void* a, int a_dtype, const void* x, int x_dtype, void* out, int out_dtype, int B, int n, int Ca, int Cb, int64_t HW, void* stream);
int vs_cat_bcast_bwd(const void* dout, int dout_dtype, void* da, int a_dtype, void* dx, int x_dtype, int B, int n, int Ca, int Cb, int64_t HW, void* stream);
int64_t vs_code_losses_chunks(int n_pairs, const int64_t* count, int64_t t_count);
int vs_code_losses_fwd(int n_pairs, const void* const* a, const void* const* b, const int* dtype, const int64_t* count, const float* t0, int64_t t_count,
                       const float* sse_ae, const float* sse_pred, float scale_ae, float scale_pred, float l_ae, float l_s, float l_pred, float l_t,
                       float inv_s, float inv_t, float* partial, float* out, void* stream);
int vs_code_losses_bwd(int n_pairs, const void* const* a, const void* const* b, void* const* da, void* const* db, const int* dtype, const int64_t* count,
                       const float* t0, float* dt0, int64_t t_count, const float* g, float scale_ae, float scale_pred, float l_ae, float l_s, float l_pred,
                       float l_t, float inv_s, float inv_t, float* coefs, void* stream);

/* dz[i] = dy[i] * act'(y[i]) evaluated from the activation OUTPUT y (see vs_gemm mask semantics).
 * Backward of the trailing activation of a chain (mlp_encdec.py:49 last_activation, conv.py:230).  */
int vs_act_bwd(const void* dy, int dy_dtype, const void* y, int y_dtype, void* dz, int dz_dtype, int act,
               int64_t n, void* stream);

/* y[i] = act(x[i]) (out of place or in place).  networks/utils.py:50-72.                             */
int vs_act_fwd(const void* x, int x_dtype, void* y, int y_dtype, int act, int64_t n, void* stream);

/* dst[c*rows + r] = (dst_dtype) src[r*cols + c]: transposed (and converted) weight copies for the backward rollout. */
int vs_transpose_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int rows, int cols, void* stream);

/* ------------------------------------------------------------------------------------------------
 * vs_mlp_rollout_{fwd,bwd}: the residual latent integrator rolled over time in one persistent launch.
 *
 * Replaces the python loop of SeparableNetwork.get_forecast (networks/model.py:78-83) around
 * MLPResnet.forward / MLPResBlock.forward (networks/resnet.py:22-50):
 *     for t in 1..n-1:  for b in blocks:  r = W3_b relu(W2_b relu(W1_b x + b1_b) + b2_b) + b3_b ;  x = x + r
 * Forward:
 *   x0        [B, C] fp32         initial temporal code (E_t output)
 *   weights   host array of 3*n_blocks device pointers {W1 [H,C], W2 [H,H], W3 [C,H]} per block, each PRE-PACKED by
 *             vs_pack_rollout_weight in the compute type;  biases: host array of 3*n_blocks fp32 device pointers
 *   t_codes   [B, n, C] fp32      every code of the rollout, t_codes[:, 0] = x0 (the layout get_forecast returns)
 *   residuals [n-1, n_blocks, B, C] fp32 or NULL   (the `t_residuals` the reference returns)
 *   xin_save [nb, n-1, B, C], h1_save / h2_save [nb, n-1, B, H]  compute type: inputs of the weight-gradient GEMMs
 *   m1_save / m2_save [nb, n-1, Bp, P, 32] uint32, Bp = B rounded up to 16, P = vs_mlp_rollout_parts(...): ReLU sign
 *             bits of h1 / h2, opaque to the caller (written by _fwd, read by _bwd of the same sizes), so the backward
 *             kernel reads a few words per step instead of the activations
 *   workspace: exchange area of vs_mlp_rollout_workspace_bytes(...) bytes, ZERO-FILLED ONCE by the caller when it creates it and then
 *             left to the library (the weight-stationary form numbers its launches through per-slab epoch words inside it and
 *             never clears it; the slab form clears it itself; an all-zero area is always a valid state); its last 16 bytes hold a
 *             timeout flag.  bf16, C <= 32, H in {128, 256, 512}, ceil(B/16) * n_blocks * H/64 <= 224: weight-stationary
 *             pipelined form -- one workgroup per (16-row slab, block, 64-column part) keeps its weight fragments in
 *             registers for the whole rollout and hands [16, C] partials to the workgroups of the next block through
 *             the exchange area.  Otherwise the slab form:  When the hidden size
 *             allows it the H x H layer of every 16-row slab is split over P workgroups (P CUs stream 1/P of the
 *             weights each); they all-reduce one [16, C] partial per block-step through this area with epoch-tagged
 *             8-byte granules (placement independent, bounded spins).  NULL / too small => P = 1 (no split).
 * Backward (through time):
 *   grad_t_codes [B, n, C] fp32   gradient wrt every code;  weights_t: host array of 3*n_blocks device pointers
 *             {W3^T [H,C], W2^T [H,H], W1^T [C,H]} per block, packed with vs_pack_rollout_weight(transpose = 1)
 *   dx0 [B, C] fp32; dr_save [nb, n-1, B, C], dh2_save / dh1_save [nb, n-1, B, H] compute type.
 *   Weight gradients are then vs_gemm(dh1_save[b] (S), xin_save[b] (S)) etc. with K = (n-1)*B, bias gradients
 *   vs_colsum of the same buffers.
 * P workgroups per 16 batch rows; partial sums are combined in a fixed order: results are bitwise reproducible.
 * Limits: n_blocks <= 8; LDS footprint (grows with H) must fit 160 KiB (H <= ~2048 in bf16).
 */
/* Pre-pack of one integrator weight for the rollout kernels: the logical matrix L[N][K] (L = src if transpose == 0,
 * with src fp32 [N,K];  L = src^T if transpose == 1, with src fp32 [K,N]) is converted to the compute type and laid
 * out in MFMA-fragment order, one contiguous 1 KiB piece per (16-column tile, k-step), zero padded, so that every
 * wave-level weight load of the rollout is a single fully coalesced 1 KiB read.  dst must hold
 * vs_rollout_packed_elems(compute, N, K) elements of the compute type.  Re-run after each optimizer step.          */
size_t vs_rollout_packed_elems(int compute, int N, int K);
int vs_pack_rollout_weight(int compute, const float* src, int transpose, int N, int K, void* dst, void* stream);
/* The same for several weights in one launch (<= 48 jobs): src[i] fp32 [rows, cols], logical L = src or src^T [N[i], K[i]]. */
int vs_pack_rollout_weights(int compute, int n_jobs, const float* const* src, const int* transpose, const int* N, const int* K,
                            void* const* dst, void* stream);

int vs_mlp_rollout_parts(int compute, int B, int C, int H);
size_t vs_mlp_rollout_workspace_bytes(int compute, int B, int C, int H);
/* Round 5: the exchange mode of the weight-stationary integrator (reference resnet.py:22-50 unrolled over time, model.py:74-86) is a
 * START-UP decision.  With 8 / 16 / ... row slabs the ring of a slab publishes its granules with plain stores that only reach ONE XCD's
 * L2: it leans on a dispatch property HIP does not promise (workgroups 8 apart share an XCD).
 *   _get   1 when a launch of this geometry would take the XCD-local stores now (VS_ROLLOUT_XCD_LOCAL != 0, 8 k slabs, not refused)
 *   _set   0: agent-scope (sc1) stores for the rest of the process -- what the caller does when its probe rollout (a first launch with a
 *          short spin limit on a fresh workspace) came back with the error word raised; 1: allow again
 * VS_ROLLOUT_XCD_LOCAL=2 (test aid) keeps the plain stores but deals the slabs out so that every ring is spread over the XCDs.            */
int vs_mlp_rollout_xcd_local_get(int compute, int B, int C, int H, int n_blocks);
int vs_mlp_rollout_xcd_local_set(int allowed);
/* The exchange guard: ONE 4-byte device word (caller-owned, zero = fine) registered for the process.  While registered, every kernel with
 * a bounded in-launch exchange (vs_mlp_rollout_fwd / _bwd: bit 1; vs_conv3_img16_bn_fwd / _bwd: bit 2) raises this word on a time-out
 * INSTEAD of the word inside its own workspace, and every optimizer launch issued afterwards (vs_adam_multi, vs_adam_multi_scaled,
 * vs_gemm_adam, vs_adam_step_increment*) reads it first and leaves parameters, moments, operand copies and the step count untouched
 * while it is non-zero (the pointer is taken when a launch is issued or recorded): `optimizer.step()` (reference train.py:156-158) never
 * applies an update computed from a timed-out exchange.  The caller reads and clears the word (it is sticky).  NULL unregisters.        */
int vs_exchange_guard_set(void* word);
void* vs_exchange_guard_get(void);
/* Optional companion of the guard: a second caller-owned 4-byte device word that vs_adam_step_increment* bumps by one every time the guard
 * made it skip a step (reference train.py:156-158: `optimizer.step()` did not happen), so that the host can report HOW MANY steps a sticky
 * time-out cost between two reads.  NULL unregisters; the caller reads and clears it.                                                     */
int vs_exchange_skip_counter_set(void* word);
int vs_mlp_rollout_fwd(int compute, int B, int C, int H, int n_blocks, int n_steps, const float* x0,
                       const void* const* weights, const float* const* biases, float* t_codes, float* residuals,
                       void* xin_save, void* h1_save, void* h2_save, uint32_t* m1_save, uint32_t* m2_save, void* workspace,
                       size_t workspace_bytes, void* stream);

int vs_mlp_rollout_bwd(int compute, int B, int C, int H, int n_blocks, int n_steps, const float* grad_t_codes,
                       const void* const* weights_t, const void* h1_save, const void* h2_save,
                       const uint32_t* m1_save, const uint32_t* m2_save, float* dx0,
                       void* dr_save, void* dh2_save, void* dh1_save, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Convolutions as im2col-free implicit GEMMs on NCHW tensors (csrc/vs_conv.hip).  x [B,Cin,H,W], stride/pad equal
 * in both directions, dilation 1, groups 1 -- the only forms the reference uses.  Storage type of x / w / dy is the
 * compute type; biases and weight gradients are fp32.
 *
 *   vs_conv2d_*            nn.Conv2d          w [Cout,Cin,kh,kw]   y [B,Cout,OH,OW], OH = (H + 2 pad - kh)/stride + 1
 *                          conv.py:119-122 (k4 s2 p1), :147-165,300-317,326-343,362-382,402-417 and resnet.py:57-59
 *                          (k3 s1 p1), :170 (k4 s1 p0)
 *   vs_conv_transpose2d_*  nn.ConvTranspose2d w [Cin,Cout,kh,kw]   y [B,Cout,OH,OW], OH = (H - 1) stride - 2 pad + kh
 *                          conv.py:258,295 (k4 s1 p0), :260-263 (k4 s2 p1), :318 (k3 s1 p1)
 *   *_fwd   : y = conv(x, w) + bias (bias may be NULL)
 *   *_dgrad : dx = gradient wrt x given dy (dy has the shape of y)
 *   The two TRANSPOSED-form contractions (vs_conv_transpose2d_fwd, vs_conv2d_dgrad) take `w_packed`, the weight
 *   pre-packed by vs_conv_pack_weight (channel dims swapped, taps grouped per output-parity phase for stride 2,
 *   converted to the compute type; refresh it after each optimizer step).  Supported there: stride 1 (any k, pad) and
 *   stride 2 with k - 2*pad == 2 (the reference's k4 s2 p1), run as 4 dense parity phases.
 *   *_wgrad : dw (fp32, same shape as w) = gradient wrt w; uses split-K when the reduction B*OH*OW is long: pass a
 *             workspace of vs_conv_wgrad_workspace_bytes(...) bytes (NULL = no split, slower but correct)
 * In every call B, Cin, H, W, Cout describe the FORWARD op (x's shape and the weight's channel counts).
 */
/* Workspace for every conv entry point below (forward, input gradient, weight gradient of Conv2d(Cin, Cout, k, stride, pad) on
 * [B, Cin, H, W] and of the ConvTranspose2d with the same numbers).  With a workspace of this size, contractions with >= 64
 * output channels run as "gather once into a transient column matrix, then dense MFMA GEMM" (2-3x faster than gathering
 * inside the MFMA loop); with workspace = NULL (or too small) they gather inside the loop.  The result is the same either way. */
size_t vs_conv_workspace_bytes(int compute, int B, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad);
size_t vs_conv_wgrad_workspace_bytes(int B, int Cin, int OH, int OW, int Cout, int kh, int kw);
/* w: fp32 master weight [D0][D1][kh][kw] (Conv2d: D0 = Cout, D1 = Cin; ConvTranspose2d: D0 = Cin, D1 = Cout);
 * dst: vs_conv_packed_elems(...) elements of the compute type.                                                     */
size_t vs_conv_packed_elems(int D0, int D1, int kh, int kw, int stride, int pad);
int vs_conv_pack_weight(int compute, const float* w, int D0, int D1, int kh, int kw, int stride, int pad, void* dst, void* stream);
int vs_conv2d_fwd(int compute, const void* x, const void* w, const float* bias, void* y, int y_dtype, int B, int Cin, int H, int W,
                  int Cout, int kh, int kw, int stride, int pad, void* workspace, size_t workspace_bytes, void* stream);
int vs_conv2d_dgrad(int compute, const void* dy, const void* w_packed, void* dx, int dx_dtype, int B, int Cin, int H, int W, int Cout, int kh,
                    int kw, int stride, int pad, void* workspace, size_t workspace_bytes, void* stream);
int vs_conv2d_wgrad(int compute, const void* dy, const void* x, float* dw, int B, int Cin, int H, int W, int Cout, int kh, int kw,
                    int stride, int pad, void* workspace, size_t workspace_bytes, void* stream);
/* The weight gradients with an `accumulate` flag: dw += (non-zero) instead of dw =.  A module applied many times per step
 * (ConvResBlock inside the rollout loop of model.py:78-83: one call per predicted frame) adds each call's contribution in the
 * GEMM / split-K epilogue instead of a separate add launch per call and parameter.                                          */
int vs_conv2d_wgrad_acc(int compute, const void* dy, const void* x, float* dw, int B, int Cin, int H, int W, int Cout, int kh, int kw,
                        int stride, int pad, void* workspace, size_t workspace_bytes, int accumulate, void* stream);
int vs_conv_transpose2d_wgrad_acc(int compute, const void* dy, const void* x, float* dw, int B, int Cin, int H, int W, int Cout, int kh,
                                  int kw, int stride, int pad, void* workspace, size_t workspace_bytes, int accumulate, void* stream);
int vs_conv_transpose2d_fwd(int compute, const void* x, const void* w_packed, const float* bias, void* y, int y_dtype, int B, int Cin, int H,
                            int W, int Cout, int kh, int kw, int stride, int pad, void* workspace, size_t workspace_bytes, void* stream);
int vs_conv_transpose2d_dgrad(int compute, const void* dy, const void* w, void* dx, int dx_dtype, int B, int Cin, int H, int W, int Cout,
                              int kh, int kw, int stride, int pad, void* workspace, size_t workspace_bytes, int cols_from_wgrad, void* stream);
int vs_conv_transpose2d_wgrad(int compute, const void* dy, const void* x, float* dw, int B, int Cin, int H, int W, int Cout, int kh,
                              int kw, int stride, int pad, void* workspace, size_t workspace_bytes, void* stream);

/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1) on `planes` = B*C planes of H x W (reference: conv.py:517, the ResNet18
 * stem of the chairs encoder); output (H + 2 - 3) / 2 + 1 per side.  Backward gathers over the overlapping windows (arg-max =
 * first maximum in window order, as ATen), no atomics.                                                                  */
int vs_maxpool3s2_fwd(const void* x, int x_dtype, void* y, int y_dtype, int64_t planes, int H, int W, void* stream);
int vs_maxpool3s2_bwd(const void* x, int x_dtype, const void* dy, int dy_dtype, void* dx, int dx_dtype, int64_t planes, int H, int W,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm2d + activation, pooling, upsampling (csrc/vs_norm.hip); x is NCHW [B,C,HW], dtypes VS_F32 | VS_BF16.
 *
 * GROUPS: the batch of B samples is `groups` consecutive groups of B/groups samples and every group is normalised
 *                 with its own statistics -- one group per reference CALL.  This is what lets the n+1 decoder calls of
 *                 a training step (model.py:74-83) run as one batch over time with exactly the reference's per-call
 *                 BatchNorm semantics.  mean / invstd / dgamma / dbeta are [groups, C] (sum dgamma/dbeta over groups).
 * vs_bn_stats   : per-call batch statistics of nn.BatchNorm2d in training mode (conv.py:41-60): mean[g][c], invstd[g][c]
 *                 = 1/sqrt(biased var + eps); when running_mean/var are non-NULL they are updated in place, group by
 *                 group in call order, with `momentum` and the unbiased variance, exactly like `groups` sequential ATen
 *                 calls (var_scratch: [groups, C] floats).
 * vs_bn_act_fwd : y = act(gamma (x - mean) invstd + beta).  Eval mode: pass running_mean and 1/sqrt(running_var+eps).
 * vs_bn_act_bwd : given dy = dL/dy, recomputes z = gamma xhat + beta, dz = dy act'(z), and returns dbeta = sum dz,
 *                 dgamma = sum dz xhat and dx = gamma invstd (dz - dbeta/N - xhat dgamma/N)  (training != 0) or
 *                 dx = gamma invstd dz (training == 0).
 * vs_chan_sum   : out[c] = sum_{b,pix} x[b,c,pix]   (bias gradient of a convolution)
 * vs_maxpool2_* : nn.MaxPool2d(2,2) (conv.py:151-169,330-335) on `planes` = B*C planes of H x W (even); backward
 *                 routes dy to the first maximum in window scan order, like ATen.
 * vs_upsample2_*: nn.Upsample(scale_factor=2, mode='nearest') (conv.py:296-314,371-377,406-413); H, W are the INPUT size.
 */
int vs_bn_stats(const void* x, int x_dtype, int B, int C, int64_t HW, int groups, float* mean, float* invstd, float* var_scratch,
                float* running_mean, float* running_var, float momentum, float eps, void* stream);
/* Training-mode BatchNorm2d + activation of ONE reference call on a small tensor (slabs B*HW <= 8192 per channel: the SST
 * integrator's 8 x 16 x 16 maps, conv.py:41-60 blocks inside resnet.py:53-88) in one launch: statistics, running-statistics update
 * (momentum, unbiased variance; NULL = not tracked), y = act(gamma * x_hat + beta); mean / invstd [C] are kept for vs_bn_act_bwd.
 * vs_bn_train_fwd_small_supported tells whether a tensor is served (else: vs_bn_stats + vs_bn_act_fwd, same results up to summation
 * order).  vs_bn_act_bwd takes the matching one-launch path by itself.                                                      */
int vs_bn_train_fwd_small_supported(int x_dtype, int B, int C, int64_t HW);
int vs_bn_train_fwd_small(const void* x, int x_dtype, void* y, int y_dtype, const float* gamma, const float* beta, int act, float* mean,
                          float* invstd, float* running_mean, float* running_var, float momentum, float eps, int B, int C, int64_t HW,
                          void* stream);
/* the same for `groups` calls stacked along the batch axis (per-call statistics, mean / invstd [groups][C]); var_scratch [groups][C] is needed when
 * running statistics are tracked (they are folded in call order by a second launch) */
int vs_bn_train_fwd_small_groups(const void* x, int x_dtype, void* y, int y_dtype, const float* gamma, const float* beta, int act, float* mean,
                                 float* invstd, float* var_scratch, float* running_mean, float* running_var, float momentum, float eps, int B, int C,
                                 int64_t HW, int groups, void* stream);
/* vs_bn_train_fwd_small on the split slabs of vs_conv3_img16: z = round(sum of the slabs + bias[c]) in the 16-bit z_dtype is written
 * (vs_bn_act_bwd needs it), everything else as above.  skip / xnew (fp32, both or neither) and xnew16 (z_dtype, optional): the tail of
 * a residual block (ConvResBlock.forward resnet.py:66-70) -- xnew = skip + y and its 16-bit copy for the next block.           */
int vs_bn_train_fwd_small_slabs(const float* slabs, int nslabs, const float* bias, void* z, int z_dtype, void* y, int y_dtype, const float* gamma,
                                const float* beta, int act, float* mean, float* invstd, float* running_mean, float* running_var,
                                float momentum, float eps, const float* skip, float* xnew, void* xnew16, int B, int C, int64_t HW,
                                void* stream);
/* Backward of the same block in one launch (training mode, one call, 16-bit z): the upstream gradient is the sum of split slabs
 * (slabs != NULL: what a vs_conv3_img16 input-gradient launch left) or dy_a (+ dy_b, fp32: the two outputs of a residual block,
 * resnet.py:66-70); accumulate != 0 adds d gamma / d beta to the vectors given (the parameter's pending gradient of this pass).  */
int vs_bn_act_bwd_small_ex(const void* dy_a, int dy_a_dtype, const float* dy_b, const float* slabs, int nslabs, const void* z, int z_dtype,
                           const float* mean, const float* invstd, const float* gamma, const float* beta, int act, float* dgamma,
                           float* dbeta, int accumulate, void* dx, int dx_dtype, int B, int C, int64_t HW, void* stream);
/* Round 4: training-mode BatchNorm2d (+ activation) forward with every (call group, channel) slab read ONCE (reference conv.py:41-60): slabs of
 * 8 193 .. 131 072 16-bit elements live in the registers of a 1024-thread workgroup between the statistics and the apply phase (vs_bn_stats +
 * vs_bn_act_fwd read the tensor twice).  mean / invstd [groups][C]; running estimates folded in call order (groups > 1: var_scratch [groups][C]).
 * The backward counterpart (x and dy resident, slabs up to 65 536 elements) is taken by vs_bn_act_bwd / _gsum by itself. */
int vs_bn_train_fwd_slab_supported(int x_dtype, int Bg, int C, int64_t HW);
int vs_bn_train_fwd_slab(const void* x, int x_dtype, void* y, int y_dtype, const float* gamma, const float* beta, int act, float* mean, float* invstd,
                         float* var_scratch, float* running_mean, float* running_var, float momentum, float eps, int B, int C, int64_t HW, int groups,
                         void* stream);
int vs_bn_act_fwd(const void* x, int x_dtype, void* y, int y_dtype, const float* mean, const float* invstd, const float* gamma,
                  const float* beta, int act, int B, int C, int64_t HW, int groups, void* stream);
int vs_bn_act_bwd(const void* dy, int dy_dtype, const void* x, int x_dtype, const float* mean, const float* invstd, const float* gamma,
                  const float* beta, int act, int training, int groups, float* dgamma, float* dbeta, void* dx, int dx_dtype, int B,
                  int C, int64_t HW, void* stream);
/* vs_bn_act_bwd that additionally returns the PARAMETER gradients, i.e. dgamma / dbeta summed over the call groups ([C] each; with the
 * n + 1 decoder calls of a step stacked, nn.BatchNorm2d's weight receives the sum of n + 1 per-call gradients, conv.py:41-60): written
 * by workgroup 0 of the apply pass (or one small launch behind the one-launch form) instead of two reduction launches by the caller.   */
int vs_bn_act_bwd_gsum(const void* dy, int dy_dtype, const void* x, int x_dtype, const float* mean, const float* invstd, const float* gamma,
                       const float* beta, int act, int training, int groups, float* dgamma, float* dbeta, void* dx, int dx_dtype, int B,
                       int C, int64_t HW, float* dgamma_sum, float* dbeta_sum, void* stream);
/* vs_bn_stats + vs_bn_act_fwd with the running-statistics fold moved INTO the apply pass (one launch less per BatchNorm call): vs_bn_stats_ub leaves the
 * unbiased variances in ubvar [groups][C]; vs_bn_act_fwd_running applies mean / invstd and folds (mean, ubvar) into running_mean / running_var in call order */
int vs_bn_stats_ub(const void* x, int x_dtype, int B, int C, int64_t HW, int groups, float* mean, float* invstd, float* ubvar, float eps, void* stream);
int vs_bn_act_fwd_running(const void* x, int x_dtype, void* y, int y_dtype, const float* mean, const float* invstd, const float* gamma, const float* beta,
                          int act, int B, int C, int64_t HW, int groups, const float* ubvar, float* running_mean, float* running_var, float momentum,
                          void* stream);
int vs_chan_sum(const void* x, int x_dtype, int B, int C, int64_t HW, float* out, void* stream);
/* the same sum with per-chunk partial sums in a workspace of vs_chan_sum_workspace_bytes: no atomics (a 1-channel map serialises 1024 of them on
 * one address), fixed summation order */
size_t vs_chan_sum_workspace_bytes(int B, int C, int64_t HW);
int vs_chan_sum_ws(const void* x, int x_dtype, int B, int C, int64_t HW, void* ws, size_t ws_bytes, float* out, void* stream);
int vs_maxpool2_fwd(const void* x, int x_dtype, void* y, int y_dtype, int64_t planes, int H, int W, void* stream);
int vs_maxpool2_bwd(const void* x, int x_dtype, const void* dy, int dy_dtype, void* dx, int dx_dtype, int64_t planes, int H, int W,
                    void* stream);
int vs_upsample2_fwd(const void* x, int x_dtype, void* y, int y_dtype, int64_t planes, int H, int W, void* stream);
int vs_upsample2_bwd(const void* dy, int dy_dtype, void* dx, int dx_dtype, int64_t planes, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VARSEP_HIP_H */
