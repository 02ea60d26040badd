/*
 * crlot_dsp.h -- C ABI of the MI355X (gfx950) batched STFT -> iSTFT -> OLA engine.
 *
 * Replaces, for the hot path, the reference's host objects (file:line in
 * /root/reference):
 *   dsp::Framer                  dsp/frame/framer.h:26-127, framer.cc:15-181
 *   dsp::WindowLUT               dsp/window/WindowLUT.h:80-287, WindowLUT.cc:215-388
 *   dsp::fft::IFftPlan           dsp/fft/api/fft_api.h:16-51,
 *                                dsp/fft/backends/kissfft_adapter.cc:11-269
 *   dsp::OLAAccumulator          dsp/ola/OLAAccumulator.h:15-217, OLAAccumulator.cc:13-295
 *   dsp::ola::build_norm_linear  dsp/ola/norm_builder.cc:8-52
 *   axpy_windowed / normalize_and_clear   dsp/ola/kernels.cc:18-52
 * and the round trip the harness assembles from them
 * (bench/e2e_benchmark.cc:138-186, streaming-interleaved order: push frame k,
 * then produce(H)).
 *
 * Conventions: plain C types only.  Device pointers (d_*) are caller-owned HIP
 * device memory; host pointers are plain host memory.  `stream` is a hipStream_t
 * passed as void* (NULL = default stream).  Every entry returns 0 on success or
 * a negative CRLOT_E* code; crlot_last_error() gives the message of the last
 * failure on the calling thread.  Nothing throws across this boundary.
 * Streams and threads: a plan may serve several HIP streams at once.  Its
 * launch scratch (K_pair's regime flags, the staged path's frame workspace, the
 * interleaved path's channel planes) is kept per stream handle, so round trips
 * issued on different streams never share device scratch, and growth is
 * stream-ordered (hipMallocAsync / hipFreeAsync on the calling stream: no
 * device-wide synchronisation).  Host-side entry points take the plan's lock,
 * so several host threads may also share a plan (the reference's KissFftPlan
 * is non-reentrant: kissfft_adapter.cc:256-263).  Streaming objects
 * (crlot_stream*, crlot_stream_rt*, crlot_ola*) are single-owner objects.
 * The composite entries -- crlot_spectrogram where it is staged,
 * crlot_time_stretch, crlot_pitch_shift, crlot_griffin_lim, crlot_hpss_masks,
 * crlot_hpss and crlot_convolve (on the convolver's engine plan) -- keep their
 * workspace (spectra, medians, masks, staged frames, chunk sums, uncropped
 * outputs) in the calling stream's slot too, carved anew by every call; the
 * staged crlot_roundtrip, crlot_stft and crlot_istft_ola and the chunked
 * crlot_phase_vocoder carve the same buffer.  Nothing in it outlives the call
 * that wrote it, and a call that needs more frees and reallocates it in stream
 * order, behind the work already queued.  A plan keeps 16 slots: a call on a
 * further stream takes over the least recently used one, and that one call
 * waits for the whole device (hipDeviceSynchronize) before it frees the slot's
 * buffers, since the evicted stream may have work in flight; a plan used from
 * at most 16 streams never waits.
 * Stream capture: once the stream's slot exists and is large enough -- after
 * one call of the same shape on that stream (or crlot_plan_reserve_stream for
 * the round trips), which also runs each launcher's one-time queries --
 * crlot_roundtrip, crlot_spectrogram, crlot_time_stretch, crlot_pitch_shift,
 * crlot_griffin_lim, crlot_hpss and crlot_convolve only launch kernels and asynchronous
 * device-to-device copies and may be captured into a HIP graph and replayed;
 * crlot_convolve and crlot_pitch_shift need crlot_convolver_prepare /
 * crlot_resampler_prepare (or any earlier call) first, because the first use
 * uploads the filter with synchronous copies.  A call that has to create,
 * grow or recycle a slot must not be captured.
 */
#ifndef CRLOT_DSP_H_
#define CRLOT_DSP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRLOT_ABI_VERSION 2

/* error codes */
#define CRLOT_OK 0
#define CRLOT_EINVAL (-1)       /* bad argument (reference: std::invalid_argument) */
#define CRLOT_EUNSUPPORTED (-2) /* valid for the reference, not on this device path */
#define CRLOT_EHIP (-3)         /* HIP runtime error */
#define CRLOT_ENOMEM (-4)       /* allocation failed (reference: std::bad_alloc) */
#define CRLOT_ERUNTIME (-5)     /* reference: std::runtime_error */
#define CRLOT_ERANGE (-6)       /* reference: std::out_of_range */

/* dsp::WindowType (WindowLUT.h:14-20) */
#define CRLOT_WIN_HANN 0
#define CRLOT_WIN_HAMMING 1
#define CRLOT_WIN_BLACKMAN 2
#define CRLOT_WIN_RECT 3
#define CRLOT_WIN_BLACKMAN_HARRIS 4 /* rejected, as in WindowLUT.cc:241-242 */
/* dsp::NormalizationType (WindowLUT.h:25-31) */
#define CRLOT_NORM_NONE 0
#define CRLOT_NORM_SUM_TO_ONE 1
#define CRLOT_NORM_L2 2
#define CRLOT_NORM_OLA_UNITY_GAIN 3
#define CRLOT_NORM_OLA_SUM_WSQ 4
/* framing source: dsp::BoundaryMode (framer.h:11-14) of a whole-stream Framer
 * push, or dsp::FrameQueue (FrameQueue.h:26-96) with center / pad_mode */
#define CRLOT_ZERO_PAD 0
#define CRLOT_DROP 1
#define CRLOT_FRAMEQUEUE 2
/* dsp::PadMode (FrameQueue.h:8-12) */
#define CRLOT_PAD_CONSTANT 0
#define CRLOT_PAD_REFLECT 1
#define CRLOT_PAD_EDGE 2

typedef struct crlot_plan crlot_plan;
typedef struct crlot_stream crlot_stream;

/* Plan description: the union of OLAConfig (OLAAccumulator.h:15-29), the
 * Framer parameters (framer.h:46-47) and the window choice of the harness
 * (e2e_benchmark.cc:48-64).  Zero-initialise, then set the fields. */
typedef struct crlot_plan_desc {
    int32_t frame_size;          /* N: even, <= 16384 (powers of two 256..4096 run the
                                    register-resident kernels, other sizes the mixed-radix path) */
    int32_t hop_size;            /* H: 1..N */
    int32_t window_type;         /* CRLOT_WIN_* */
    int32_t periodic;            /* 0 = symmetric (reference default) */
    int32_t window_norm;         /* CRLOT_NORM_* */
    int32_t boundary_mode;       /* CRLOT_ZERO_PAD / CRLOT_DROP (Framer) or CRLOT_FRAMEQUEUE */
    int32_t analysis_window;     /* 1: frame * w before forward (e2e_benchmark.cc:154-156) */
    int32_t apply_window_inside; /* OLAConfig::apply_window_inside */
    float eps;                   /* OLAConfig::eps; 0 -> 1e-8f */
    float ola_gain;              /* push_frame_AoS gain; 0 -> 1.0f */
    int32_t ring_len;            /* 0 -> (ceil(N/H)+20)*H (OLAAccumulator.cc:249-258) */
    int32_t device;              /* HIP device ordinal, -1 = current */
    int32_t center;              /* CRLOT_FRAMEQUEUE: pad N/2 both sides (FrameQueue default: 1) */
    int32_t pad_mode;            /* CRLOT_FRAMEQUEUE: CRLOT_PAD_* */
} crlot_plan_desc;

const char* crlot_last_error(void);
int crlot_abi_version(void);
/* What this binary was built from: "src:<hash> arch:gfx950", the hash being
 * tools/src_hash.py's lib_hash() of the library's sources at build time (a
 * prebuilt library older than the tree it ships in shows a different hash). */
const char* crlot_build_info(void);

/* ---------------------------------------------------------------- plan */
int crlot_plan_create(const crlot_plan_desc* desc, crlot_plan** out);
void crlot_plan_destroy(crlot_plan* plan);
/* Replace the plan's window (N floats) and/or COLA norm table (ring_len floats)
 * with host-built ones (NULL keeps the plan's own, which are built on the host
 * by the reference formulas, bit-exact). */
int crlot_plan_upload_tables(crlot_plan* plan, const float* window, const float* norm);
/* Spectral hook between rfft and irfft: real per-bin gain, N/2+1 host floats;
 * NULL restores the identity step of the reference (e2e_benchmark.cc:161-162). */
int crlot_plan_set_spectral_gain(crlot_plan* plan, const float* gain);
/* Stream-ordered forms of the two table updates: the host data is staged in
 * pinned memory and copied with hipMemcpyAsync on `stream`, so work enqueued on
 * `stream` before the call sees the old tables and work after it the new ones
 * (the host arrays may be reused as soon as the call returns).  The stream-less
 * entries above first drain the device (hipDeviceSynchronize), so a round trip
 * in flight on any stream never reads a half-updated table. */
int crlot_plan_upload_tables_async(crlot_plan* plan, const float* window, const float* norm,
                                   void* stream);
int crlot_plan_set_spectral_gain_async(crlot_plan* plan, const float* gain, void* stream);
/* Frame pairing on the fused round trip (default on): two consecutive frames
 * (2j, 2j+1) of a stream share one complex FFT, z = frame_2j + i frame_2j+1,
 * whose real and imaginary round-trip outputs are the two frames' (exact for
 * the real, bin-symmetric spectral gain).  Used where those kernels exist
 * (N = 512, 1024, 2048, 4096 with the fused hop rules); a pair holding a NaN, Inf,
 * huge or tiny sample is transformed frame by frame instead, so no frame's
 * overflow reaches its neighbour.  Results equal the per-frame kissfft
 * formulation within float32 rounding, not bit for bit, and do not depend on
 * the batch or the chunking.  0 selects the per-frame (kiss_fftr split)
 * kernels, bit-identical to crlot_roundtrip_stages + crlot_ola_gather.  2 keeps
 * pairing but runs the power-of-two pair kernels' two-regime walkers on every
 * chunk (their paired-only hot walkers off): bit-identical to 1, for parity
 * diagnostics.  Other values: CRLOT_EINVAL. */
int crlot_plan_set_frame_pairing(crlot_plan* plan, int32_t enable);
/* Chunks per stream the chunked walkers of crlot_roundtrip /
 * crlot_roundtrip_interleaved split every stream into (every frame-pair walker
 * and the per-frame fused walkers).  0 (default) lets the library choose (whole
 * resident rounds of the device); n > 0 forces min(n, F) chunks (min(n, F/2) on
 * the two-wave K_pairN walks).  Output bits never depend on it (each chunk
 * recomputes its warm-up frames); it exists so parity tests can move the chunk
 * seams, and the launch record below reports the chunking a call used.
 * Negative: CRLOT_EINVAL. */
int crlot_plan_set_chunks(crlot_plan* plan, int32_t chunks_per_stream);
/* Speculation of the host-pointer drop-in calls (IFftPlan forward / inverse,
 * OLAAccumulator push / produce), process-wide.  1: each forward also computes
 * the inverse and the produce block that follow it on the call kernel.  2
 * (default): in addition, when a forward's input is bit for bit the frame a
 * dsp::Framer just popped times a window table the library built (or the
 * dsp::FrameQueue frame read last), the loop over that signal runs as batches
 * on the device, windows of at most `window_frames` frames
 * (crlot_call_batch_capacity), and the following calls are served from them
 * after a bitwise check of each call's input and arguments; an inverse input
 * that is the served spectrum times a fixed real gain per bin teaches the batch
 * that gain.  The first call that differs otherwise ends the batch and the OLA
 * object's ring is rebuilt from the frames it was served; a batch that cannot
 * allocate or launch declines and the call takes its ordinary path.  Results
 * are the same bits in both modes.  Other values: CRLOT_EINVAL. */
int crlot_set_call_speculation(int32_t mode);
/* Process-wide counters of the batched speculation: [0] batches started, [1]
 * forwards, [2] inverses, [3] pushes, [4] produces served from a batch, [5] OLA
 * rings rebuilt after a call the batch did not predict. */
int crlot_call_speculation_stats(int64_t* out6);
/* The same counters and more, out[0 .. count): [0..5] as above, [6] frames the
 * batches transformed, [7] window continuations (a batch is bounded: at most
 * `window_frames` frames per chain, below; the next window starts at the
 * forward of the first frame past it), [8] speculations declined because a
 * buffer or launch failed (the call then took the ordinary path), [9] spectral
 * gains learned (an inverse input that was the served spectrum times a fixed
 * real gain per bin, bit for bit: the batch's remaining inverses are then those
 * of the gained spectra, each still served only after a bitwise check), [10]
 * learned gains not applied because the previous one served fewer than four
 * inverses and differed in more than an eighth of the bins (a time-varying
 * edit: those frames take the per-call path, learning backs off for 16, 32, ..
 * frames); entries past the known ones are 0.  Negative: CRLOT_EINVAL. */
int crlot_call_speculation_stats_ex(int64_t* out, int32_t count);
/* Bounds of the batched speculation: frames per window, and the device and
 * pinned host bytes the batches hold now, with the pinned peak since load. */
int crlot_call_batch_capacity(int64_t* window_frames, int64_t* device_bytes, int64_t* pinned_bytes,
                              int64_t* pinned_peak);
/* Test-only fault injection: CRLOT_INJECT_BATCH_ALLOC makes the next `count`
 * buffer allocations of the batched speculation fail (a speculation that cannot
 * allocate declines and the call takes its ordinary path);
 * CRLOT_INJECT_CALL_TIMEOUT makes the next `count` waits on the resident call
 * kernel take their timeout path (the call fails with CRLOT_EHIP; the server
 * serves again once every request submitted before completed).  Other `what`:
 * CRLOT_EINVAL. */
#define CRLOT_INJECT_BATCH_ALLOC 1
#define CRLOT_INJECT_CALL_TIMEOUT 2
int crlot_test_inject(int32_t what, int32_t count);
/* What the plan's last call on `stream` launched: kernels in launch order
 * (CRLOT_K_* ids below; the first 8 are kept, n_kernels counts all), the
 * workgroups of each launch, and the chunks per stream of the walk (0 when the
 * call ran no chunked walker).  Recorded by crlot_roundtrip,
 * crlot_roundtrip_interleaved, crlot_roundtrip_stages, crlot_ola_gather and
 * the batched FFTs; a call that failed records what it launched before failing.
 * No call on `stream` yet: n_kernels = 0. */
#define CRLOT_K_PAIR_HOT 1       /* K_pair paired-only walker, N = 1024 */
#define CRLOT_K_PAIR_FIX 2       /* K_pair two-regime walker: the flagged chunks after the hot walker */
#define CRLOT_K_PAIR_ALL 3       /* K_pair two-regime walker over every chunk */
#define CRLOT_K_PAIR512_HOT 4
#define CRLOT_K_PAIR512 5        /* two-regime walker, N = 512 (flagged chunks or all, see fix_all) */
#define CRLOT_K_PAIR2K_HOT 6
#define CRLOT_K_PAIR2K 7
#define CRLOT_K_PAIR4K_HOT 8
#define CRLOT_K_PAIR4K 9
#define CRLOT_K_FUSED 10         /* per-frame fused walker, one frame per wave in flight */
#define CRLOT_K_FUSED2 11        /* ... two frames per wave in flight */
#define CRLOT_K_FUSED_WG 12      /* per-frame workgroup walker, N = 4096 */
#define CRLOT_K_PAIR15 13        /* N = 960 / 480 pairs */
#define CRLOT_K_PAIRN 14         /* N = 320 ... 1764 pairs (2, 3, 5, 7 factors) */
#define CRLOT_K_PAIR30 15        /* N = 1920 pairs, even hops */
#define CRLOT_K_FUSED_ANY 16     /* any-size per-frame walker (all streams, or the flagged ones) */
#define CRLOT_K_SYNTH 17         /* staged path: frames */
#define CRLOT_K_SYNTH_ANY 18
#define CRLOT_K_GATHER 19        /* staged path: overlap-add gather */
#define CRLOT_K_DEINTERLEAVE 20
#define CRLOT_K_INTERLEAVE 21
#define CRLOT_K_FFT 22           /* batched rfft / irfft / cfft */
#define CRLOT_K_FFT_ANY 23
#define CRLOT_K_STFT 24          /* crlot_stft: x -> spectra */
#define CRLOT_K_ISTFT 25         /* crlot_istft_ola: spectra -> step -> y */
#define CRLOT_K_STFT_MASKED 26   /* crlot_roundtrip with a spectral mask: one walk x -> y */
#define CRLOT_K_SPEC_STEP 27     /* staged spectral step (gain, mask) over spectra in HBM */
#define CRLOT_K_FRAMES_W 28      /* staged windowed frames (mixed-radix stft) */
#define CRLOT_K_PAIR_MASK 29     /* N = 1024 frame-pair walk with the per-frame mask */
#define CRLOT_K_PAIR_STFT 30     /* crlot_stft as frame pairs (N = 1024) */
#define CRLOT_K_PAIR_ISTFT 31    /* crlot_istft_ola as frame pairs (N = 1024) */
#define CRLOT_K_FEAT 32          /* crlot_spectrogram: one frame per wave (N = 256 / 512 / 1024) */
#define CRLOT_K_PAIR_FEAT 33     /* crlot_spectrogram as frame pairs (N = 1024) */
#define CRLOT_K_FEAT_STEP 34     /* crlot_spectrogram, staged: features of spectra in HBM */
#define CRLOT_K_PHASE_VOC 35     /* crlot_phase_vocoder: spectra -> time-stretched spectra */
#define CRLOT_K_PHASE_VOC_SUMS 36 /* ... the per-chunk phase increment sums, ahead of it when the walk is chunked */
#define CRLOT_K_RESAMPLE_PHASE 37 /* crlot_resample: one lane per filter phase, its taps in registers */
#define CRLOT_K_RESAMPLE_ANY 38  /* crlot_resample: one lane per output, any filter length */
#define CRLOT_K_GL_PROJECT 39   /* crlot_gl_project: the Griffin-Lim projection over spectra in HBM */
#define CRLOT_K_GL_ITER 40      /* crlot_griffin_lim: one fused iteration y_i -> y_i+1 (N = 256 / 512 / 1024) */
/* (41 is not assigned: crlot_kernel_name(41) stays "unknown") */
#define CRLOT_K_HPSS_FREQ 42    /* crlot_hpss_masks: the running median along frequency */
#define CRLOT_K_HPSS_TIME 43    /* crlot_hpss_masks: the running median along time, then the masks */
/* (44 is not assigned: crlot_kernel_name(44) stays "unknown") */
#define CRLOT_K_FDL_MAC 45      /* crlot_fdl_mac: the frequency-domain delay line of crlot_convolve */
/* (46 is not assigned: crlot_kernel_name(46) stays "unknown") */
#define CRLOT_K_SCONV_HEAD 47   /* crlot_stream_convolve_hop: the hop, the chain's last term (or all of it), block k */
#define CRLOT_K_SCONV_TAIL 48   /* ... the next frame's partial chain, off the critical path */
#define CRLOT_K_FDAF_HOP 49     /* crlot_fdaf_hop: filter, error, power estimate, error spectrum and gradient */
#define CRLOT_K_FDAF_UPDATE 50  /* ... the weight update over the partitions */
#define CRLOT_K_FDAF_CONSTRAIN 51 /* ... the gradient constraint (crlot_fdaf_constrain) */
/* (52 is not assigned: crlot_kernel_name(52) stays "unknown") */
#define CRLOT_K_DENOISE_GAINS 53 /* crlot_denoise_gains: the suppressor's gains over spectra in HBM, a lane per column */
#define CRLOT_K_DENOISE_HOP 54  /* crlot_stream_denoise_hop, fused: the hop with the gain computed in the mask row's place */
#define CRLOT_K_STREAM_STFT 55  /* ... staged: the hop's analysis half (crlot_stream_stft_hop's kernel) */
#define CRLOT_K_STREAM_ISTFT 56 /* ... staged: the synthesis half with the gains as its mask row */
#define CRLOT_K_XSPEC_ACC 57    /* crlot_xspec_accumulate: the four averaged planes over two spectra, a lane per column */
#define CRLOT_K_XSPEC_DERIVE 58 /* crlot_xspec_derive: coherence, H1 and the weighted cross-spectrum from a state block */
#define CRLOT_K_XSPEC_PEAK 59   /* crlot_xspec_peak: the arg-max over the lags of a correlation row, a wave per pair */
#define CRLOT_K_BF_ACC 60       /* crlot_beamform_accumulate: the two spatial covariance matrices per bin, a lane per matrix column */
#define CRLOT_K_BF_SOLVE 61     /* crlot_beamform_solve: loading, Cholesky and the MVDR weights of a bin in registers */
#define CRLOT_K_BF_APPLY 62     /* crlot_beamform_apply: y = w^H x per frame, the weights of a bin in registers */
#define CRLOT_K_BF_HOP 63       /* crlot_stream_beamform_hop: one frame's update, the solve when due and the apply */
#define CRLOT_K_WPE_POWER 64    /* crlot_wpe_power: the inverse power row of a group's frames, a lane per column */
#define CRLOT_K_WPE_ACC 65      /* crlot_wpe_accumulate: the stacked correlation matrices per bin, a lane per 4 x 4 tile */
#define CRLOT_K_WPE_SOLVE 66    /* crlot_wpe_solve: loading, Cholesky and the taps of a bin, in place on workspace planes */
#define CRLOT_K_WPE_FILTER 67   /* crlot_wpe_filter: the prediction filter along the frames, a lane per (column, microphone) */
#define CRLOT_K_WPE_GAIN 68     /* crlot_wpe_rls: v = Q y~ of one frame, a wave per row of Q */
#define CRLOT_K_WPE_UPDATE 69   /* crlot_wpe_rls: the update of Q by rows, the prediction and the taps' update */
#define CRLOT_K_EXPERIMENT 99   /* experiment builds only */
typedef struct crlot_launch_info {
    int32_t n_kernels;
    int32_t kernels[8];
    int64_t grid[8];
    int32_t n_chunks;
    int32_t reserved;
} crlot_launch_info;
int crlot_plan_last_launch(const crlot_plan* plan, void* stream, crlot_launch_info* out);
/* Name of a CRLOT_K_* id ("k_pair_hot", ...); "unknown" otherwise. */
const char* crlot_kernel_name(int32_t kernel_id);
int crlot_plan_info(const crlot_plan* plan, int32_t* frame_size, int32_t* hop_size,
                    int32_t* ring_len);
/* Frames of a T-sample stream: Framer whole push (framer.cc:88-117) or
 * FrameQueue::calculateNumFrames on the padded length (FrameQueue.cc:98-115) */
int64_t crlot_frame_count(const crlot_plan* plan, int64_t T);
/* Samples the streaming-interleaved round trip emits: F*H */
int64_t crlot_output_length(const crlot_plan* plan, int64_t T);
/* Device workspace a non-fast-path crlot_roundtrip needs (bytes); reserve it
 * up front so the launch itself never allocates (graph capture).
 * crlot_plan_reserve grows the default (NULL) stream's slot and waits for it;
 * crlot_plan_reserve_stream grows `stream`'s slot (regime flags, frame
 * workspace, channel planes) for round trips of n_streams groups of `channels`
 * channels (1 = crlot_roundtrip) of T samples, stream-ordered. */
int64_t crlot_workspace_bytes(const crlot_plan* plan, int32_t n_streams, int64_t T);
int crlot_plan_reserve(crlot_plan* plan, int64_t bytes);
int crlot_plan_reserve_stream(crlot_plan* plan, int32_t n_streams, int64_t T, int32_t channels,
                              void* stream);

/* ---------------------------------------------------------------- hot path */
/* The round trip for n_streams independent mono streams: stream s reads
 * d_x[s*ld_x + t], t < T, and writes d_y[s*ld_y + n], n < crlot_output_length.
 * Equals, per stream, Framer(push whole) -> pop -> *w -> IFftPlan::forward ->
 * (spectral hook) -> IFftPlan::inverse -> OLAAccumulator::push_frame_AoS(k*H)
 * -> produce(H), frame after frame.  With CRLOT_FRAMEQUEUE the frames are
 * FrameQueue(x, T, N, H, center, pad_mode).getFrame(k) (output sample n is at
 * padded position n) -- the performance_benchmark.cc:174-246 pipeline, with
 * analysis_window = 0 there.  d_x may be NULL when T == 0. */
int crlot_roundtrip(crlot_plan* plan, const float* d_x, float* d_y, int32_t n_streams, int64_t T,
                    int64_t ld_x, int64_t ld_y, void* stream);

/* The same round trip for n_groups groups of `channels` interleaved channels
 * (the reference's multi-channel PCM: Framer::set_params(N, H, C) frames N*C
 * interleaved samples, push_frame_AoS deinterleaves them; framer.cc:15-35,
 * aos_to_soa.cc:7-18): group g's input is T rows of C samples at d_x + g*ld_x
 * (ld_x >= T*C), its output F*H rows of C samples at d_y + g*ld_y.  Every
 * channel is an independent stream, bit-identical to crlot_roundtrip on that
 * channel's plane.  N = 1024 plans with zero padding walk the interleaved rows
 * of up to 5 channels directly (K_pair with strided hop loads and stores: one
 * pass over HBM); other plans and wider rows run LDS-tiled deinterleave -> the
 * mono kernels -> interleave through a plan-owned workspace of
 * n_groups*C*(T + F*H) floats (two extra HBM passes). */
int crlot_roundtrip_interleaved(crlot_plan* plan, const float* d_x, float* d_y, int32_t n_groups,
                                int32_t channels, int64_t T, int64_t ld_x, int64_t ld_y, void* stream);

/* Per-stage outputs of the same path (parity/debug): d_frames gets, per
 * stream and frame, the N-sample push_frame_AoS input (sanitized inverse
 * output, before the synthesis window), [s][k][N]; d_spec (optional) the
 * forward spectrum [s][k][N/2+1] complex (float pairs). */
int crlot_roundtrip_stages(crlot_plan* plan, const float* d_x, int32_t n_streams, int64_t T,
                           int64_t ld_x, float* d_frames, float* d_spec, void* stream);

/* OLAAccumulator over precomputed frames: d_frames [s][k][ld_frames] (k < F)
 * pushed at k*H with the plan's synthesis window (apply_window_inside) and
 * gain, normalised by max(norm, eps) and produced in H-sample steps:
 * d_y[s*ld_y + n], n < F*H.  Bit-exact with the reference given equal frames. */
int crlot_ola_gather(crlot_plan* plan, const float* d_frames, float* d_y, int32_t n_streams,
                     int64_t F, int64_t ld_frames, int64_t ld_y, void* stream);

/* ---------------------------------------------------------------- the spectral step
 * The round trip split where the reference's harness leaves its spectral
 * processing step (e2e_benchmark.cc:160-162, identity there), so any
 * device-side processing -- masks, Wiener gains, a model -- can sit between
 * the halves with the spectra in HBM.
 *
 * crlot_stft: the analysis half.  Per stream and frame (framing exactly as
 * crlot_roundtrip: Framer ZERO_PAD / DROP or FrameQueue), frame * analysis
 * window, then IFftPlan::forward (sanitize, kiss_fftr; kissfft_adapter.cc
 * :83-122): spectrum k of stream s, N/2+1 complex bins as float pairs, at
 * d_spec[s*ld_spec + k*ld_frame + 2*b], b <= N/2.  ld_frame >= N+2 floats;
 * d_spec 8-byte aligned, ld_frame and ld_spec even.  F = crlot_frame_count(T)
 * frames per stream.  With frame pairing 0: bit-identical to
 * crlot_rfft_batched on the windowed frames.
 *
 * crlot_istft_ola: the synthesis half.  Spectra in that layout (F frames per
 * stream) -> the plan's spectral step (the per-bin gain of
 * crlot_plan_set_spectral_gain, then row k of the mask below) ->
 * IFftPlan::inverse (kiss_fftri, *1/N, sanitize; kissfft_adapter.cc:124-168)
 * -> push_frame_AoS(k*H) with the synthesis window and gain -> produce(H)
 * (OLAAccumulator.cc:124-221): d_y[s*ld_y + n], n < F*H.  With frame pairing 0:
 * bit-identical to crlot_irfft_batched of the stepped spectra +
 * crlot_ola_gather.  The imaginary parts of bins 0 and N/2 are ignored, as
 * kiss_fftri ignores them.
 *
 * With frame pairing on (the default) these entries and the masked
 * crlot_roundtrip run frames (2j, 2j+1) through one complex transform where the
 * pair kernels exist, and the bit identities above become float32 tolerances:
 *   - results are within float32 rounding of the per-frame formulation
 *     (per stream rel-L2 1e-6, max-abs 4e-6 max|x|);
 *   - block by block, the error of output block b is at most 4e-6 times the
 *     largest inverse-transform output among the frames that overlap it AND
 *     their pair mates (k ^ 1): a quiet frame may carry rounding noise of its
 *     loud mate, never of a frame further away;
 *   - a gated frame stays silent: a frame whose stepped spectrum (istft_ola) or
 *     whose multiplier row gain * mask (masked round trip) is all zero is
 *     inverted alone when its mate is not, so an output block all of whose
 *     frames are gated is exactly +0, as with pairing 0;
 *   - likewise a frame of exact zeros in x next to a live one is transformed
 *     alone by crlot_stft and the masked crlot_roundtrip (its spectrum is exact
 *     zeros, whatever mask attenuates its mate);
 *   - the unmasked crlot_roundtrip (the hot pair walkers) keeps no such
 *     exception: exact silence in x before an onset may carry up to 4e-6 times
 *     the onset frame's scale for one hop.
 *
 * crlot_plan_set_spectral_mask: a time-varying spectral step.  Row (s, k) of
 * N/2+1 real floats at d_mask[s*ld_stream + k*ld_frame] multiplies frame k of
 * stream s after the per-bin gain (ld_stream = 0: one row per frame, shared by
 * every stream).  Device memory owned by the caller, read by every later
 * crlot_roundtrip, crlot_roundtrip_interleaved (stream = channel plane
 * g*C + c) and crlot_istft_ola on the plan until it is replaced or cleared
 * (NULL); it must hold a row for every frame those calls run (nothing here
 * checks its extent: the Python binding does, before the call).  With a mask
 * and frame pairing 0,
 * crlot_roundtrip(x) equals crlot_istft_ola(crlot_stft(x)) bit for bit (one
 * walk over HBM where the shape allows it: power-of-two N, H % 128 == 0,
 * N % H == 0, 8-byte aligned output rows).  The per-hop streaming object takes
 * its mask a row per call (crlot_stream_push_hop_masked, crlot_stream_istft_hop)
 * and never reads the plan's; the resident crlot_stream_rt, the host-pointer calls
 * and crlot_roundtrip_stages keep the per-bin gain only. */
int crlot_plan_set_spectral_mask(crlot_plan* plan, const float* d_mask, int64_t ld_frame, int64_t ld_stream);
int crlot_stft(crlot_plan* plan, const float* d_x, float* d_spec, int32_t n_streams, int64_t T, int64_t ld_x,
               int64_t ld_spec, int64_t ld_frame, void* stream);
int crlot_istft_ola(crlot_plan* plan, const float* d_spec, float* d_y, int32_t n_streams, int64_t F,
                    int64_t ld_spec, int64_t ld_frame, int64_t ld_y, void* stream);

/* ---------------------------------------------------------------- spectrogram features
 * crlot_stft's analysis half with the feature computed where the spectrum
 * would be stored: |X|^2, |X| or filterbank bands of them, optionally logged.
 * The complex spectra never reach HBM where crlot_stft itself would run its
 * per-wave kernel at N = 256 / 512 / 1024 or its frame-pair kernel at N = 1024
 * (H = 128 / 256 / 512).  Every other route of crlot_stft stages the spectra
 * through a bounded workspace, same values: N = 2048 / 4096, the mixed-radix
 * sizes, and N = 512 at H = 128 / 256 under the default frame pairing (its stft
 * is the N = 512 frame-pair kernel; with pairing 0 it takes the per-wave walker).
 *
 * The value contract.
 *   Per bin.  X[b] is bit for bit what crlot_stft writes for that frame under the
 *   plan's current frame-pairing setting (no sanitize after the forward).  Then
 *     p = fl(fl(re*re) + fl(im*im))     two products and one sum, each rounded to
 *                                       float32, no FMA; +Inf when it overflows
 *     CRLOT_FEAT_MAGNITUDE: sqrtf(p), correctly rounded.
 *   Filterbank.  At creation row j is reduced to its span [lo, hi): the first to
 *   the last non-zero weight (crlot_filterbank_spans; an all-zero row has
 *   lo = hi = 0 and yields +0 before the log).  Only the spans' weights live on
 *   the device.  With v the per-bin value of the chosen kind,
 *     band j = sum over b in [lo, hi) of fl(w[j][b] * v[b])
 *   in float32, in this order, fixed per (N, band):
 *     - span offset i = b - lo belongs to part g = i mod 8; part g adds its terms
 *       t_i = fl(w_i * v_i) in ascending i starting from +0:
 *       s_g = (((0 + t_g) + t_{g+8}) + t_{g+16}) + ...   (every sum rounded, no FMA);
 *     - band = ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)).
 *   Every kernel runs this one order, so output bits never depend on batch size,
 *   chunking, stream count, ld_*, the kernel chosen (walker or staged) or the
 *   run.  No float atomics.
 *   Log.  The value logged is bit for bit the LIN output: logf / log10f /
 *   10 * log10f of fmaxf(v, floor); a NaN value logs as floor.
 *
 * desc.floor is read only when log != CRLOT_FEAT_LIN and must then be finite and
 * >= FLT_MIN.  weights: host [n_bands][N/2+1] row-major, NULL iff n_bands == 0,
 * every weight finite.  The plan must outlive the object; several objects may
 * share a plan.  crlot_spectrogram takes the plan's lock and records its
 * kernels in crlot_plan_last_launch (CRLOT_K_FEAT / _PAIR_FEAT / _FEAT_STEP;
 * n_chunks reported as crlot_stft reports it: equal to crlot_stft's under
 * crlot_plan_set_chunks; the library's own choice follows the residency of the
 * kernel that runs and may differ).  The staged form slices the streams so that its
 * workspace (spectra, and the windowed frames of mixed-radix sizes) stays within
 * 256 MiB, or one stream's worth if that is more. */
#define CRLOT_FEAT_POWER 0      /* re*re + im*im */
#define CRLOT_FEAT_MAGNITUDE 1  /* sqrt of that */
#define CRLOT_FEAT_LIN 0
#define CRLOT_FEAT_LN 1         /* logf(max(v, floor)) */
#define CRLOT_FEAT_LOG10 2
#define CRLOT_FEAT_DB 3         /* 10 * log10f(max(v, floor)) */
typedef struct crlot_features crlot_features;
typedef struct crlot_features_desc {
    int32_t kind;     /* CRLOT_FEAT_POWER / _MAGNITUDE */
    int32_t n_bands;  /* 0: one value per bin, n_out = N/2+1; 1..512: filterbank rows, n_out = n_bands */
    int32_t log;      /* CRLOT_FEAT_LIN / _LN / _LOG10 / _DB */
    float floor;      /* log != LIN: finite and >= FLT_MIN; a NaN value logs as floor (fmaxf) */
} crlot_features_desc;
/* weights: host [n_bands][N/2+1] row-major, NULL iff n_bands == 0; the plan must outlive the object */
int crlot_features_create(crlot_plan* plan, const crlot_features_desc* desc, const float* weights,
                          crlot_features** out);
void crlot_features_destroy(crlot_features* f);
/* any of the outputs may be NULL; widest_band: the longest span (0 without a filterbank) */
int crlot_features_info(const crlot_features* f, int32_t* n_out, int32_t* kind, int32_t* log_mode,
                        int32_t* widest_band);
/* frame k of stream s (framing, window, sanitize, forward exactly as crlot_stft): n_out floats at
 * d_out[s*ld_out + k*ld_frame + j]; ld_frame >= n_out; F = crlot_frame_count(T).  F == 0 or
 * n_streams == 0: CRLOT_OK, nothing written. */
int crlot_spectrogram(crlot_features* f, const float* d_x, float* d_out, int32_t n_streams, int64_t T,
                      int64_t ld_x, int64_t ld_out, int64_t ld_frame, void* stream);

/* ---------------------------------------------------------------- time stretch
 * The phase vocoder (librosa.phase_vocoder, torchaudio.functional.phase_vocoder)
 * between crlot_stft and crlot_istft_ola: F frames in, F' frames out, duration
 * changed by 1/rate, pitch kept.  rate is a finite double in [1/64, 64];
 * rate > 1 shortens the signal.  Anything else is CRLOT_EINVAL.
 *
 * The time axis.
 *   tau_t = (double)t * rate                     one IEEE double multiply
 *   F' = crlot_stretch_frame_count(F, rate)      the number of t >= 0 with tau_t < F (this
 *                                                predicate, not ceil(F / rate): the two differ by
 *                                                one at some rates); F = 0 -> 0; F < 0, a bad
 *                                                rate or F' > 2^31-1 -> CRLOT_EINVAL
 *   i_t = floor(tau_t),  alpha_t = (float)(tau_t - i_t)
 *   A frame with index >= F is all zeros and is never loaded from memory.
 *   crlot_stretch_output_length(plan, T, rate) = F'(crlot_frame_count(T)) * H.
 *
 * The values, per stream and bin, X[k] being frame k of the input with both
 * components sanitized on load as IFftPlan's sanitize does (NaN / Inf -> 0,
 * |v| < 1e-30 -> 0):
 *   q(z)  the phase of z in units of 2^-32 turn, a 32-bit integer modulo 2^32:
 *           rint(fl(atan2f(im, re) * fl(2^32 / 2 pi))), 2^31 wrapping to -2^31; q(0) = 0
 *           (fl(pi) * fl(1 / 2 pi) is exactly 1/2 in float32, so a negative real is exactly 2^31)
 *   m(z)  sqrtf(fl(fl(re*re) + fl(im*im))), the CRLOT_FEAT_MAGNITUDE value (no FMA)
 *   acc_0     = q(X[0])
 *   acc_{t+1} = acc_t + q(X[i_t + 1]) - q(X[i_t])            wrapping 32-bit integer arithmetic
 *   mag_t     = fl(fl(alpha_t * m(X[i_t + 1])) + fl(fl(1 - alpha_t) * m(X[i_t])))
 *   out_t     = (mag_t * cos phi, mag_t * sin phi),  phi = 2 pi acc_t / 2^32
 *               (the nearest quarter turn comes off acc_t in integers, exactly; the rest
 *               goes through float32 radians: cos and sin are good to about 1.2e-7)
 *   Bins 0 and N/2: input imaginary parts are ignored (taken as 0), output
 *   imaginary parts are stored as +0.
 * This is the librosa / torchaudio recurrence: their expected phase advance and
 * the wrap to [-pi, pi] cancel modulo 2 pi, so the result does not depend on the hop.
 * The integer accumulator has two consequences:
 *   - the sum is associative and wraps a turn for free, so the output bits do not
 *     depend on how the time axis is split into chunks (crlot_plan_set_chunks),
 *     nor on n_streams, a stream's position in the batch or the leading dimensions;
 *   - the phase error does not grow with the size of the accumulated phase, as it
 *     does in a float32 cumulative sum; it grows with the number of steps alone
 *     (each q is good to a few 2^-24 turn).
 * Domain: magnitudes are exact to float32 rounding for components in
 * {0} or [2^-60, 2^60] in size; beyond that re*re + im*im may overflow and m
 * becomes +Inf (and the outputs Inf / NaN), or underflow to 0.  The float ->
 * integer conversion only ever sees finite values of at most 2^31 in size.
 *
 * crlot_phase_vocoder: spectra in crlot_stft's layout on both sides -- bin b of
 * frame k of stream s at d[s*ld_spec + k*ld_frame + 2*b], ld_frame >= N+2 floats,
 * both leading dimensions even, base 8-byte aligned -- with independent leading
 * dimensions; F frames per stream in, F' out.  The buffers must not overlap
 * (CRLOT_EINVAL when the ranges intersect).  F = 0 or n_streams = 0: CRLOT_OK,
 * nothing written.  F > 2^31-1: CRLOT_EUNSUPPORTED, as crlot_stft.  One lane owns
 * one (stream, bin) column and walks its output frames in order with 64-bit
 * addressing (no 2^27 / 2^29 extent limits).  A batch too small to fill the
 * device splits [0, F') into chunks: CRLOT_K_PHASE_VOC_SUMS writes each chunk's
 * increment sum per column into the stream's scratch slot and CRLOT_K_PHASE_VOC
 * starts each chunk from the wrapped sum of the chunks before it;
 * crlot_plan_set_chunks(n) forces min(n, F') chunks, crlot_plan_last_launch
 * reports the kernels and n_chunks.
 *
 * crlot_time_stretch is by definition
 * crlot_istft_ola(crlot_phase_vocoder(crlot_stft(x))) on the plan, bit for bit:
 * framing is the plan's; the plan's gain and stored mask apply to the stretched
 * frames (a mask must hold F' rows; the Python binding checks this before the
 * call); it writes d_y[s*ld_y + n] for n < F' * H.  The spectra live in the
 * stream's scratch slot; the streams are processed in slices whose workspace
 * (both spectra and the staged routes' frames) stays within 256 MiB, or one
 * stream's worth if that is more.  crlot_plan_last_launch lists the last
 * slice's kernels in launch order (the analysis half's, CRLOT_K_PHASE_VOC_SUMS
 * when that slice's walk is chunked, CRLOT_K_PHASE_VOC, the synthesis half's);
 * its n_chunks is that of the last chunked walk among them. */
int64_t crlot_stretch_frame_count(int64_t F, double rate); /* host only, no device */
int64_t crlot_stretch_output_length(const crlot_plan* plan, int64_t T, double rate);
int crlot_phase_vocoder(crlot_plan* plan, const float* d_spec_in, float* d_spec_out, int32_t n_streams,
                        int64_t F, double rate, int64_t ld_spec_in, int64_t ld_frame_in,
                        int64_t ld_spec_out, int64_t ld_frame_out, void* stream);
int crlot_time_stretch(crlot_plan* plan, const float* d_x, float* d_y, int32_t n_streams, int64_t T,
                       double rate, int64_t ld_x, int64_t ld_y, void* stream);
/* ---------------------------------------------------------------- resample / pitch shift
 * A batched, band-limited rational resampler: the polyphase windowed-sinc design
 * of torchaudio.functional.resample, from rate `down` to rate `up`.
 *
 * Object.  crlot_resampler_create checks the descriptor, builds the table on the
 * host and touches no device; the table is uploaded to desc.device by the first
 * call that needs it (a blocking copy; crlot_resampler_prepare does it ahead of
 * time, e.g. before a stream capture).  The object is standalone: it needs no
 * plan.  It is thread-safe behind its own mutex, as plans are.
 *   up, down   new and original rate, both >= 1
 *   zeros      1..64: zero crossings of the sinc kept on either side
 *   rolloff    in [0.5, 1]: the cutoff as a share of the lower Nyquist rate
 *   window     CRLOT_RESAMPLE_HANN or CRLOT_RESAMPLE_KAISER
 *   beta       Kaiser only: finite, in [0, 20]
 *   device     device index, >= 0
 * Reduction and limits.  U = up / gcd and D = down / gcd must both lie in
 * 1..4096 and U / D in [1/64, 64]; anything else is CRLOT_EINVAL.
 * Filter geometry.  base = min(U, D) * rolloff, W = ceil(zeros * D / base),
 * K = 2 W taps.  A table of more than 2^21 floats (U * K) is CRLOT_EUNSUPPORTED.
 * Table.  The host builds it in double and rounds each entry once to float32:
 *   h[r][i] for r in [0, U), i in [0, K):  j = i - W + 1,  tau = (j - r/U) * base / D,
 *   h = (base / D) * sinc(tau) * win(tau) where |tau| < zeros, +0 elsewhere;
 *   sinc(tau) = sin(pi tau) / (pi tau), 1 at tau = 0;
 *   Hann:   win = cos^2(pi tau / (2 zeros));
 *   Kaiser: win = I0(beta * sqrt(1 - (tau / zeros)^2)) / I0(beta).
 * crlot_resampler_table copies the U x K table, row-major, to host memory;
 * crlot_resample_table_host builds it from a descriptor without an object.
 * Length.  L = crlot_resample_output_length(r, T) = (T * U + D - 1) div D; T = 0
 * gives 0; T < 0 or T > 2^48 is CRLOT_EINVAL.
 * Values.  For output m of a stream:
 *   c = (m * D) div U and r = (m * D) mod U, in 64-bit integers;
 *   acc = +0; for i = 0 .. K-1, in that order: acc = fmaf(h[r][i], xs[c - W + 1 + i], acc);
 *   y[m] = acc + (+0.0f)   (a zero output is always +0, so an implementation that
 *                           pads the table with zero taps stays bit-identical);
 *   xs[k] is x[k] sanitized as everywhere else in this library (NaN / Inf -> 0,
 *   |v| < 1e-30 -> 0), and 0 for k outside [0, T): such samples are never loaded.
 * Invariance.  Every output is an independent chain in a fixed order, so the
 * output bits do not depend on the tiling, the batch, a stream's position, the
 * leading dimensions or the route.
 *
 * crlot_resample writes d_y[s*ld_y + m] for m < L.  The buffers must not overlap
 * (CRLOT_EINVAL); ld_x >= T; ld_y >= L when n_streams > 1.  T = 0 or
 * n_streams = 0: CRLOT_OK, nothing written.  Addressing is 64-bit throughout:
 * no 2^27 / 2^29 extent limits.  More than 2^31-1 workgroups in one call is
 * CRLOT_EUNSUPPORTED.
 *
 * Kernels.  CRLOT_K_RESAMPLE_PHASE while a table row fits in registers (K <= 104,
 * U <= 512 and one block's input span fits the tile's LDS budget): a lane owns
 * one phase and walks the output blocks q of its tile, m = q U + r.
 * CRLOT_K_RESAMPLE_ANY for every other shape: one lane per output.  Both stage
 * the tile's input span in LDS, sanitized once, and run the same tap order.
 * Test knobs: crlot_resampler_set_route (CRLOT_RESAMPLE_PHASE on a shape it
 * cannot take: CRLOT_EUNSUPPORTED), crlot_resampler_set_tile (n output blocks of
 * U outputs per tile, clamped to what the LDS budget holds; 0: the library's
 * choice), crlot_resampler_last_launch (the object's last launch on any stream).
 *
 * crlot_rational_approx: the best rational num / den to `ratio` with
 * den <= max_den, by continued fractions with the final semiconvergent choice:
 * exactly Python's fractions.Fraction(ratio).limit_denominator(max_den).  Host
 * only.  CRLOT_EINVAL: a non-finite or non-positive ratio, one outside
 * [2^-31, 2^31), max_den < 1, or a numerator beyond 2^31-1.
 *
 * crlot_pitch_shift multiplies the pitch by D / U and keeps the length.  By
 * definition, with rate = (double)U / (double)D:
 *   z = crlot_time_stretch(x, rate), of length Ls = crlot_stretch_output_length(plan, T, rate);
 *   y[m] = crlot_resample(z)[m] for m < min(L(Ls), T), +0 for the rest up to T
 *   (librosa's fix_length), bit for bit.
 * T outputs per stream; ld_x >= T, ld_y >= T when n_streams > 1.  A rate outside
 * time stretch's [1/64, 64] is CRLOT_EINVAL, as is a plan and a resampler on
 * different devices.  The plan's gain and stored mask apply to the stretched
 * frames, exactly as in crlot_time_stretch.  z lives in the stream's scratch
 * slot behind time stretch's workspace; streams go in slices so that the whole
 * workspace stays within 256 MiB, or one stream's worth if that is more.
 * crlot_plan_last_launch lists the last slice's time-stretch kernels followed by
 * the resample kernel. */
#define CRLOT_RESAMPLE_HANN 0
#define CRLOT_RESAMPLE_KAISER 1
#define CRLOT_RESAMPLE_AUTO 0
#define CRLOT_RESAMPLE_PHASE 1
#define CRLOT_RESAMPLE_ANY 2
typedef struct crlot_resampler crlot_resampler;
typedef struct crlot_resampler_desc {
    int32_t up, down;
    int32_t zeros;
    int32_t window;
    double rolloff;
    double beta;
    int32_t device;
    int32_t reserved;
} crlot_resampler_desc;
typedef struct crlot_resampler_geometry {
    int32_t up, down;     /* U, D: reduced */
    int32_t half_width;   /* W */
    int32_t taps;         /* K = 2 W */
    int32_t phase_ok;     /* 1 when CRLOT_K_RESAMPLE_PHASE takes the shape */
    int32_t device;
} crlot_resampler_geometry;
typedef struct crlot_resample_launch {
    int32_t kernel;        /* CRLOT_K_RESAMPLE_PHASE / _ANY; 0: no launch yet */
    int32_t threads;       /* per workgroup */
    int64_t grid;          /* workgroups */
    int64_t tile_outputs;  /* outputs per tile */
    int32_t tile;          /* output blocks per tile (0: a tile is part of a block) */
    int32_t groups;        /* phase kernel: groups of U phases per workgroup */
    int32_t taps_padded;   /* phase kernel: the register bucket */
    int32_t lds_table;     /* any kernel: 1 when the table is staged in LDS */
    int64_t lds_bytes;
} crlot_resample_launch;
int crlot_resample_geometry(const crlot_resampler_desc* desc, crlot_resampler_geometry* out); /* host only */
int crlot_resample_table_host(const crlot_resampler_desc* desc, float* out /* [U][K] */);     /* host only */
int crlot_rational_approx(double ratio, int32_t max_den, int32_t* num, int32_t* den);         /* host only */
int crlot_resampler_create(const crlot_resampler_desc* desc, crlot_resampler** out);
void crlot_resampler_destroy(crlot_resampler* r);
int crlot_resampler_info(const crlot_resampler* r, crlot_resampler_geometry* out);
int crlot_resampler_table(const crlot_resampler* r, float* host_out /* [U][K] */);
int crlot_resampler_prepare(crlot_resampler* r);
int64_t crlot_resample_output_length(const crlot_resampler* r, int64_t T);
int crlot_resampler_set_route(crlot_resampler* r, int32_t route);
int crlot_resampler_set_tile(crlot_resampler* r, int32_t n_blocks);
int crlot_resampler_last_launch(const crlot_resampler* r, crlot_resample_launch* out);
int crlot_resample(crlot_resampler* r, const float* d_x, float* d_y, int32_t n_streams, int64_t T,
                   int64_t ld_x, int64_t ld_y, void* stream);
int crlot_pitch_shift(crlot_plan* plan, crlot_resampler* r, const float* d_x, float* d_y, int32_t n_streams,
                      int64_t T, int64_t ld_x, int64_t ld_y, void* stream);

/* ---------------------------------------------------------------- Griffin-Lim
 * From magnitudes back to audio: the fast Griffin-Lim iteration of librosa.griffinlim
 * / torchaudio.transforms.GriffinLim around the plan's crlot_stft and
 * crlot_istft_ola.
 *
 * The projection, per stream, frame and bin.  X is the rebuilt spectrum, T the
 * previous rebuilt spectrum (absent on the first iteration or with momentum 0),
 * m the target magnitude.  Every operation is one correctly rounded float32
 * operation, no FMA:
 *   alpha = (float)((double)momentum / (1.0 + (double)momentum))      momentum in [0, 1)
 *   c   = (X.re - fl(alpha*T.re), X.im - fl(alpha*T.im))              (c = X when T is absent)
 *   p   = fl(fl(c.re*c.re) + fl(c.im*c.im))
 *   d   = fl(sqrtf(p) + 1e-16f)                                       sqrtf correctly rounded
 *   s   = m / d                                                       IEEE division
 *   out = (fl(c.re*s), fl(c.im*s))
 * X and T are sanitized on load as IFftPlan's sanitize does (NaN / Inf -> 0,
 * |v| < 1e-30 -> 0), and so is m; a negative m is used as it is.  Bins 0 and N/2
 * take the imaginary parts of X and T as 0 and store +0.  This is torchaudio's /
 * librosa's update, angles = rebuilt - tprev * momentum / (1 + momentum);
 * angles /= |angles| + 1e-16; spec = mag * angles, with one division instead of two.
 * Domain: exact to float32 rounding for components of c in {0} or [2^-60, 2^60]
 * in size and m within [2^-60, 2^60] or 0; beyond that c.re*c.re + c.im*c.im may
 * overflow (s = 0) or underflow (d = 1e-16, s up to 1e16 m).
 *
 * crlot_gl_project applies the projection over spectra in crlot_stft's layout:
 * bin b of frame k of stream s at d[s*ld + k*ld_frame + 2*b] for d_spec, d_tprev
 * (NULL: absent) and d_out, at d_mag[s*ld_mag + k*ld_frame_mag + b] for the
 * magnitudes; every operand has its own leading dimensions; ld_frame >= N+2
 * floats for spectra (even leading dimensions, 8-byte aligned bases), >= N/2+1 for
 * d_mag.  d_out may be exactly d_spec with d_spec's leading dimensions (in
 * place); any other overlap of d_out with an input is CRLOT_EINVAL.  momentum
 * must be finite and in [0, 1).  F = 0 or n_streams = 0: CRLOT_OK, nothing
 * written.  One lane per (stream, frame, bin), 64-bit addressing
 * (CRLOT_K_GL_PROJECT).
 *
 * crlot_griffin_lim: S_0 = d_mag + 0i when d_init is NULL (the magnitudes as
 * stored: this one path does not sanitize m), else project(d_init, absent, d_mag);
 * then
 *   y_0     = istft_ola(S_0)
 *   y_{i+1} = istft_ola(project(stft(y_i), tprev_i, mag)),   tprev_{i+1} = stft(y_i)
 * for n_iter iterations (tprev_0 absent; with momentum 0 always absent), and
 * d_y[s*ld_y + n] = y_{n_iter}[n] for n < F*H.  It is by definition that
 * composition of crlot_istft_ola, crlot_stft (on F*H samples per stream) and
 * crlot_gl_project on the plan.  n_iter in [0, 65536]; momentum finite, in
 * [0, 1); the plan must frame with CRLOT_ZERO_PAD (the only mode in which
 * crlot_frame_count(F*H) == F, so the loop is closed; other modes:
 * CRLOT_EUNSUPPORTED) and must have no spectral gain and no stored mask, because
 * the projection is the spectral step (CRLOT_EINVAL otherwise).  d_init is in
 * crlot_stft's layout.  F = 0 or n_streams = 0: CRLOT_OK, nothing written.
 *
 * What it converges to.  Griffin and Lim's theorem (the distance between |stft(y_i)|
 * and d_mag never increases) holds for the least-squares inverse, whose overlap-add
 * is divided by the sum of w^2 over the frames covering a sample.  A default plan
 * divides by the reference's table, the sum of w, so with an analysis window
 * istft_ola(stft(x)) = x sum(w^2) / sum(w), every y_i is the least-squares
 * iteration's scaled by that factor (the projection reads phases only), and the
 * relative distance settles near 1 - sum(w^2) / sum(w) (0.25 for Hann at 75 %
 * overlap) instead of falling towards 0: the phases are reconstructed, the level
 * is not.  For magnitudes that approach d_mag upload sum(w^2) as the plan's norm
 * table first (crlot_plan_upload_tables; ring_len floats, periodic in H).
 *
 * Kernels.  At N = 256 / 512 / 1024 with H a multiple of 128 dividing N (and
 * ring_len % H == 0, the default) an iteration is one launch, CRLOT_K_GL_ITER:
 * K_istft's walk from y_i with the projection as its step; with momentum 0 no
 * spectrum reaches memory.  crlot_plan_set_chunks forces its chunking.  N = 1024
 * at H = 128 and 512 with momentum > 0 is not among these "fused shapes": the
 * walk measured slower than the staged iteration there.  Every other shape runs crlot_stft's dispatch, CRLOT_K_GL_PROJECT and
 * crlot_istft_ola's dispatch per iteration.  y_0 is crlot_istft_ola's dispatch.
 * Workspace (the stream's scratch slot): two y buffers, S_0 and, with momentum,
 * two rebuilt spectra, one of them in S_0's place (staged shapes: S_0's buffer holds
 * the projected rows, two more the rebuilt ones, and the staged routes' frames);
 * the streams are processed in slices whose workspace stays within 256 MiB, or
 * one stream's worth if that is more, and a slice runs all its iterations before
 * the next one starts.  crlot_plan_last_launch lists the kernels of the last
 * iteration of the last slice (of y_0 when n_iter is 0).
 *
 * Bits.  With frame pairing off the result equals the composition of the three
 * public entries bit for bit at every shape.  At the fused shapes the result does
 * not depend on the pairing setting (the walk, and y_0 there, are per-frame
 * arithmetic): with pairing on it equals the pairing-off composition bit for bit.
 * At the other shapes it equals the composition under the plan's own pairing
 * setting.  The bits never depend on chunking, the batch size, a stream's
 * position in the batch, slicing, the leading dimensions or the alignment of
 * d_y: the last step writes d_y itself only where crlot_istft_ola's dispatch takes
 * the same route into d_y as into the workspace (8-byte aligned rows an even
 * distance apart), and otherwise through the workspace.  With n_streams == 1,
 * ld_y is not read. */
int crlot_gl_project(crlot_plan* plan, const float* d_spec, const float* d_tprev, const float* d_mag, float* d_out,
                     int32_t n_streams, int64_t F, double momentum, int64_t ld_spec, int64_t ld_frame_spec,
                     int64_t ld_tprev, int64_t ld_frame_tprev, int64_t ld_mag, int64_t ld_frame_mag,
                     int64_t ld_out, int64_t ld_frame_out, void* stream);
int crlot_griffin_lim(crlot_plan* plan, const float* d_mag, int64_t ld_mag, int64_t ld_frame_mag,
                      const float* d_init, int64_t ld_init, int64_t ld_frame_init, float* d_y, int64_t ld_y,
                      int32_t n_streams, int64_t F, int32_t n_iter, double momentum, void* stream);

/* ---------------------------------------------------------------- HPSS
 * Harmonic / percussive source separation (librosa.decompose.hpss,
 * librosa.effects.hpss): two median filters over the magnitudes of spectra in
 * crlot_stft's layout (bin b of frame k of stream s at
 * d_spec[s*ld_spec + k*ld_frame + 2*b], bins = N/2+1), and from them two soft
 * masks in the layout crlot_plan_set_spectral_mask reads.
 *
 * Every step is one correctly rounded float32 operation, no FMA.
 *  1. Magnitude.  re and im are sanitized on load as IFftPlan's sanitize does
 *     (NaN / Inf -> 0, |v| < 1e-30 -> 0); the imaginary parts of bins 0 and N/2 are
 *     taken as 0;  m = sqrtf(fl(fl(re*re) + fl(im*im)))  (CRLOT_FEAT_MAGNITUDE).
 *     Domain: components in {0} or [2^-60, 2^60] in size; beyond it the formula is
 *     still evaluated literally.
 *  2. Medians.  With r = (w-1)/2 and ext(i, n) = (j = i mod 2n, 0 <= j < 2n;
 *     j < n ? j : 2n-1-j):
 *       h[k][b] = median of m[ext(k+d, F)][b],    d = -r_h .. r_h   (along time, win_harm)
 *       p[k][b] = median of m[k][ext(b+d, bins)], d = -r_p .. r_p   (along frequency, win_perc)
 *     which is scipy.ndimage.median_filter(mode='reflect'), also where the window is
 *     longer than the axis.  Windows are odd, 1 <= w <= 63 (even or non-positive:
 *     CRLOT_EINVAL; above 63: CRLOT_EUNSUPPORTED).  A median is a selection: its
 *     bits do not depend on how it is found.
 *  3. Masks.  margin_harm, margin_perc: finite doubles >= 1 (else CRLOT_EINVAL), cast
 *     once to float (mh, mp).  power is 1, 2 or CRLOT_HPSS_HARD (anything else:
 *     CRLOT_EUNSUPPORTED; powf has no bit contract).  Harmonic mask: X = h,
 *     R = fl(p*mh); percussive mask: X = p, R = fl(h*mp);
 *       Z = max(X, R)
 *       Z < FLT_MIN:  mask = (mh == 1 && mp == 1) ? 0.5f : 0      (librosa's split_zeros)
 *       else  a = X / Z, b = R / Z;  power 2: a = fl(a*a), b = fl(b*b);  mask = a / fl(a + b)
 *     CRLOT_HPSS_HARD (librosa's power = inf):  mask = X > R ? 1 : 0; a tie gives 0
 *     in both masks.
 *  4. Output.  d_mask_h[s*ld_mask_h + k*ld_frame_mask_h + b], likewise d_mask_p;
 *     ld_frame >= N/2+1; the floats between N/2+1 and ld_frame are not written.
 *
 * crlot_hpss_masks: either mask pointer may be NULL (both: CRLOT_EINVAL).  Spectra:
 * ld_frame >= N+2, even leading dimensions, an 8-byte aligned base; masks: 4-byte
 * aligned; with n_streams > 1 every stream stride covers its F rows; with
 * n_streams == 1 the stream strides are not read.  Any overlap of an output with
 * the input or with the other output is CRLOT_EINVAL.  F = 0 or n_streams = 0:
 * CRLOT_OK, nothing written.  64-bit addressing.  Kernels: CRLOT_K_HPSS_FREQ (p
 * into the stream's scratch slot, F * bins floats per stream, the streams in
 * slices under 256 MiB or one stream's worth), then CRLOT_K_HPSS_TIME (h and both
 * masks), which crlot_plan_set_chunks splits along time; the bits do not depend
 * on the split, the batch or the leading dimensions.
 *
 * crlot_hpss is by definition the composition S = crlot_stft(x); (Mh, Mp) =
 * crlot_hpss_masks(S); y_h = crlot_istft_ola(S) with Mh as the plan's spectral
 * mask; y_p likewise with Mp; F * H samples per stream and output.  It equals
 * that composition bit for bit under the plan's own pairing setting and
 * spectral gain (the gain rides as in crlot_istft_ola).  Either output may be
 * NULL (both: CRLOT_EINVAL); its mask and its inversion are then skipped.  A plan
 * with a stored mask is CRLOT_EINVAL; the call stores nothing in the plan (the
 * inversions take their mask as an argument), so host threads may run it on one
 * plan on different HIP streams.  Overlaps among x, y_h and y_p: CRLOT_EINVAL.
 * Workspace (the stream's scratch slot): the spectra, p, one mask per output and
 * the staged routes' frames; the streams go in slices under the 256 MiB cap of
 * crlot_griffin_lim, or one stream's worth if that is more.  The bits never
 * depend on slicing, chunking, the batch size, a stream's position in the batch
 * or the leading dimensions.  crlot_plan_last_launch lists the last slice's
 * kernels.  With n_streams == 1, ld_y_h and ld_y_p are not read. */
#define CRLOT_HPSS_HARD (-1) /* crlot_hpss_desc.power: the hard masks (power = inf) */
typedef struct crlot_hpss_desc {
    int32_t win_harm, win_perc; /* median windows along time / frequency: odd, 1 .. 63 (librosa: 31) */
    int32_t power;              /* 1, 2 or CRLOT_HPSS_HARD */
    int32_t reserved;           /* 0 */
    double margin_harm, margin_perc; /* finite, >= 1 */
} crlot_hpss_desc;
int crlot_hpss_masks(crlot_plan* plan, const crlot_hpss_desc* desc, const float* d_spec, float* d_mask_h,
                     float* d_mask_p, int32_t n_streams, int64_t F, int64_t ld_spec, int64_t ld_frame_spec,
                     int64_t ld_mask_h, int64_t ld_frame_mask_h, int64_t ld_mask_p, int64_t ld_frame_mask_p,
                     void* stream);
int crlot_hpss(crlot_plan* plan, const crlot_hpss_desc* desc, const float* d_x, float* d_y_h, float* d_y_p,
               int32_t n_streams, int64_t T, int64_t ld_x, int64_t ld_y_h, int64_t ld_y_p, void* stream);

/* ---------------------------------------------------------------- partitioned FFT convolution
 * Full linear convolution of every stream with a long FIR (a room response, a
 * cabinet or HRTF filter, a matched filter, a linear-phase EQ), as uniformly
 * partitioned overlap-add (torchaudio.functional.fftconvolve /
 * scipy.signal.oaconvolve give the same numbers): y[s][n] = sum_k h[q][k] x[s][n-k]
 * for n < T + K - 1, q = s mod n_filters.
 *
 * The object.  A crlot_convolver holds n_filters filters of K taps (K in
 * [1, 2^20], n_filters in [1, 65536]; host rows ld_h >= K floats apart; every tap
 * finite), cut into P = ceil(K / B) partitions of B = `block` taps, and its own
 * crlot_plan, the engine plan: N = 2B, H = B, CRLOT_ZERO_PAD, analysis_window = 1,
 * apply_window_inside = 0, ola_gain = 1, the window table replaced by B ones then B
 * zeros, the norm table by ones, no gain, no mask.  With it crlot_stft gives the
 * spectrum of every zero-padded input block (F = ceil(T / B) frames) and
 * crlot_istft_ola overlap-adds 2B-sample results.  B must make N = 2B a frame size
 * crlot_plan_create accepts (else CRLOT_EINVAL; power-of-two B in 128..2048 are
 * tested).  crlot_convolver_create touches no device: the plan is created and the
 * filter uploaded and transformed by crlot_convolver_prepare, crlot_convolver_plan
 * or the first device call.  The filter spectra are H[q][p][.] = crlot_rfft_batched
 * of block p of filter q zero-padded to N: the per-frame (kiss_fftr split)
 * transform whatever the plan's pairing setting, computed once, so toggling
 * pairing on the borrowed plan never changes H.  crlot_convolver_spectra copies
 * them to the host, [n_filters][P][N+2] floats.  crlot_convolver_plan lends the
 * engine plan (NULL on failure, crlot_last_error says why): do not destroy it, do
 * not replace its tables, gain or mask.  The object has its own lock; several host
 * threads may share it.
 *
 * crlot_fdl_mac: the frequency-domain delay line, a complex FIR along the frame
 * axis per bin.  Spectra in crlot_stft's layout on both sides (frame k of stream s
 * at d[s*ld + k*ldf + 2*b]; 8-byte aligned, even leading dimensions, ldf >= N+2).
 * Values.  For stream s, output frame f < F_out, bin b <= N/2, q = s mod n_filters:
 *   re = im = +0;
 *   for j = max(0, f-P+1) .. min(f, F_in-1), ascending, with p = f - j,
 *       (Hr, Hi) = H[q][p][b], (Xr, Xi) = X[s][j][b], in this order:
 *     re = fmaf(Hr, Xr, re);  re = fmaf(-Hi, Xi, re);
 *     im = fmaf(Hr, Xi, im);  im = fmaf(Hi, Xr, im);
 *   out[s][f][b] = (re + 0.0f, im + 0.0f).
 * Rows outside [0, F_in) are not loaded; an empty range stores +0.  X is taken as
 * it is (no sanitizing: crlot_stft's forward already mapped NaN / Inf to 0).
 * Invariance.  Every output is an independent chain in a fixed order, so its bits
 * do not depend on the frame chunking, the register tile, the batch, a stream's
 * position, the leading dimensions or the slice of crlot_convolve.  (Ascending j
 * is the order in which a sliding or per-hop implementation meets the inputs.)
 * d_spec_out must not overlap d_spec_in (CRLOT_EINVAL).  F_in >= 0, F_out >= 0;
 * F_out = 0 or n_streams = 0: CRLOT_OK, nothing written.  Only the N/2+1 bins of
 * each output row are written.  Kernel: CRLOT_K_FDL_MAC, one wave per 64 adjacent
 * bins of one stream and chunk of output frames; crlot_convolver_set_chunks forces
 * min(n, F_out) chunks per stream (0: the library's choice; a test knob),
 * crlot_convolver_last_launch reports the object's last launch on any stream.
 *
 * crlot_convolve is by definition, on the engine plan, crlot_stft(x) (F_in =
 * ceil(T / B) frames) -> crlot_fdl_mac to F_out = ceil((T + K - 1) / B) frames ->
 * crlot_istft_ola, cropped to crlot_convolve_output_length(T) = T + K - 1 samples
 * per stream (0 for T = 0), bit for bit under the engine plan's pairing and chunk
 * settings.  ld_x >= T; ld_y >= T + K - 1 when n_streams > 1 (it may be below
 * F_out B: nothing is written past sample T + K - 2 of a row).  x and y must not
 * overlap.  T = 0 or n_streams = 0: CRLOT_OK, nothing written.  Both spectra (and,
 * unless T + K - 1 is a multiple of B, the uncropped output) live in the stream's
 * scratch slot of the engine plan; streams go in slices so that this workspace
 * stays within 256 MiB, or one stream's worth if that is more.
 * crlot_plan_last_launch on the engine plan lists the last slice's kernels. */
typedef struct crlot_convolver crlot_convolver;
typedef struct crlot_convolver_desc {
    int32_t block;      /* B: N = 2B must be a frame size the plan accepts */
    int32_t n_filters;  /* >= 1; stream s uses filter s mod n_filters */
    int32_t device;     /* -1 = current */
    int32_t reserved;   /* 0 */
} crlot_convolver_desc;
typedef struct crlot_convolver_launch {
    int32_t kernel;     /* CRLOT_K_FDL_MAC; 0: no launch yet */
    int32_t threads;    /* per workgroup */
    int64_t grid;       /* workgroups */
    int32_t n_chunks;   /* chunks of output frames per stream */
    int32_t chunk;      /* output frames per chunk */
    int32_t tile;       /* output frames per register tile */
    int32_t reserved;
} crlot_convolver_launch;
int crlot_convolver_create(const crlot_convolver_desc* desc, const float* h /* host [n_filters][ld_h] */, int64_t K,
                           int64_t ld_h, crlot_convolver** out);
void crlot_convolver_destroy(crlot_convolver* c);
int crlot_convolver_info(const crlot_convolver* c, int32_t* block, int32_t* n_filters, int64_t* K, int32_t* P);
int crlot_convolver_prepare(crlot_convolver* c);
int crlot_convolver_spectra(crlot_convolver* c, float* host_out /* [n_filters][P][N+2] */);
crlot_plan* crlot_convolver_plan(crlot_convolver* c);
int64_t crlot_convolve_output_length(const crlot_convolver* c, int64_t T);
int crlot_convolver_set_chunks(crlot_convolver* c, int32_t chunks_per_stream);
int crlot_convolver_last_launch(const crlot_convolver* c, crlot_convolver_launch* out);
int crlot_fdl_mac(crlot_convolver* c, const float* d_spec_in, float* d_spec_out, int32_t n_streams, int64_t F_in,
                  int64_t F_out, int64_t ld_in, int64_t ldf_in, int64_t ld_out, int64_t ldf_out, void* stream);
int crlot_convolve(crlot_convolver* c, const float* d_x, float* d_y, int32_t n_streams, int64_t T, int64_t ld_x,
                   int64_t ld_y, void* stream);

/* ---------------------------------------------------------------- streaming convolution
 * crlot_convolve per hop, with a carried delay line: a crlot_stream_convolver over a
 * crlot_convolver (block B, P partitions, spectra H) is fed B samples per channel per
 * call, and call k writes output block k: samples [kB, (k+1)B) of the full
 * convolution of everything pushed so far with filter c mod n_filters.  The latency
 * is B samples and every call emits.  Supported blocks: B in {128, 256, 512, 1024}
 * (N = 2B on the register-resident hop kernels); any other block the convolver
 * accepts is CRLOT_EUNSUPPORTED at create.
 *
 * Values.  Output block k of channel c equals, bit for bit, samples [kB, (k+1)B) of
 * row c of crlot_convolve over the concatenated input with frame pairing off on the
 * engine plan, for the caller's blocks and for any zero blocks after them.  Per
 * channel c and hop k, q = c mod n_filters:
 *   analysis   x = sanitize(block) zero-padded to N = 2B; X_k = the per-frame forward
 *              transform and kiss_fftr split (crlot_stft's row k on the engine plan
 *              with pairing 0 = crlot_rfft_batched of the padded block), kept in row
 *              k mod P of a per-channel ring of P spectrum rows;
 *   delay line crlot_fdl_mac's chain for f = k, F_in = k + 1: from re = im = +0, for
 *              j = max(0, k-P+1) .. k ascending, p = k - j, the four fmaf in that
 *              order on H[q][p] and X_j, then + 0.0f;
 *   synthesis  kiss_fftri merge, inverse transform, * 1/N, sanitize, overlap-add as
 *              crlot_istft_ola on the engine plan (fma(fma(o, ws, 0), g, acc), then
 *              the division by the norm; ws = g = norm = 1): the first B samples plus
 *              the B samples carried from frame k-1 are block k, the last B samples
 *              the new carry.
 * d_hop_in = NULL is a block of zeros (the flush after the input ends, or a gap): the
 * bits are those of crlot_convolve, where rows j >= F_in are not loaded, because an
 * accumulator that starts at +0 never becomes -0 and adding the +-0 products of a
 * zero row to it changes nothing (H is finite: create checks the taps).  The hop
 * path has no frame pairs.
 *
 * Routes.  In frame k's chain only the last term depends on hop k.  Route 2: the hop
 * launches CRLOT_K_SCONV_HEAD, which adds that term to a partial chain formed
 * before the hop arrived, and CRLOT_K_SCONV_TAIL forms the next frame's partial
 * chain behind it, so a hop's latency does not grow with the filter.  With automatic
 * prefetch (the default) the hop enqueues the tail on the same stream; after
 * crlot_stream_convolver_set_prefetch(sc, 0) crlot_stream_convolve_prefetch does, on
 * the stream it is given (the caller orders it behind the head and in front of the
 * next hop), and a hop that finds the tail not enqueued runs it in front of its head.
 * crlot_stream_convolve_prefetch with nothing pending, or on route 1, is CRLOT_OK
 * and launches nothing.  Route 1: the head runs the whole chain, one launch, no
 * partial chain.  P = 1 is always route 1; the library's choice (route 0) is route 1
 * at P = 2 with B <= 512, where one launch measured the lower median hop, and
 * route 2 otherwise.  crlot_stream_convolver_set_route is allowed at hop 0 only, after
 * create or reset (else CRLOT_ERUNTIME).  The bits never depend on the route, the
 * prefetch mode, the channel count, a channel's position or the layout.
 *
 * The object borrows the convolver, which must outlive it; leave the engine plan's
 * tables alone.  crlot_stream_convolver_create touches no device and works on an
 * unprepared convolver (CRLOT_EINVAL: a null argument, channels < 1, a state size or
 * grid that does not fit).  crlot_stream_convolver_prepare, or the first hop,
 * prepares the convolver and allocates and zeroes the state: per channel the ring
 * [P][N+2], the partial chain [N+2] and the carry [B], floats
 * (crlot_stream_convolver_state_bytes, valid before prepare; CRLOT_ENOMEM when it does
 * not fit).  A single-owner object like crlot_stream: the hops of one object go on
 * one stream or are ordered by the caller.  Graph capture is not supported (the hop
 * index is a by-value kernel argument).  Blocks are channel-major [channels][B], or
 * [B][channels] after crlot_stream_convolver_set_layout(sc, 1).
 * crlot_stream_convolver_reset synchronises the device, zeroes the state and the hop
 * counter and clears a pending tail.  crlot_stream_convolve_hop: CRLOT_EINVAL for a
 * null sc or d_hop_out, or a d_hop_out that overlaps d_hop_in. */
typedef struct crlot_stream_convolver crlot_stream_convolver;
typedef struct crlot_sconv_launch {
    int32_t head_kernel;   /* CRLOT_K_SCONV_HEAD; 0: no hop yet */
    int32_t tail_kernel;   /* CRLOT_K_SCONV_TAIL; 0: no tail (yet) */
    int64_t head_grid;     /* workgroups: ceil(channels / 4) */
    int64_t tail_grid;     /* workgroups: channels * ceil((B + 1) / 64) */
    int32_t route;         /* 1 one launch, 2 head + tail */
    int32_t tail_pending;  /* manual prefetch: the tail of the last hop is not enqueued yet */
} crlot_sconv_launch;
int crlot_stream_convolver_create(crlot_convolver* c, int32_t channels, crlot_stream_convolver** out);
void crlot_stream_convolver_destroy(crlot_stream_convolver* sc);
int crlot_stream_convolver_prepare(crlot_stream_convolver* sc);
int64_t crlot_stream_convolver_state_bytes(const crlot_stream_convolver* sc);
int crlot_stream_convolver_reset(crlot_stream_convolver* sc);
int crlot_stream_convolver_set_layout(crlot_stream_convolver* sc, int32_t interleaved);
int crlot_stream_convolver_set_route(crlot_stream_convolver* sc, int32_t route /* 0 library's choice, 1, 2 */);
int crlot_stream_convolver_set_prefetch(crlot_stream_convolver* sc, int32_t automatic /* default 1 */);
int crlot_stream_convolver_info(const crlot_stream_convolver* sc, int32_t* channels, int32_t* block, int32_t* P,
                                int64_t* hops);
int crlot_stream_convolver_last_launch(const crlot_stream_convolver* sc, crlot_sconv_launch* out);
int crlot_stream_convolve_hop(crlot_stream_convolver* sc, const float* d_hop_in /* NULL: zeros */, float* d_hop_out,
                              void* stream);
int crlot_stream_convolve_prefetch(crlot_stream_convolver* sc, void* stream);

/* ---------------------------------------------------------------- adaptive filter
 * The partitioned-block frequency-domain adaptive filter (PBFDAF, overlap-save; Speex's
 * MDF is the best-known instance): per channel a filter of K taps, held as P =
 * ceil(K / B) weight spectra W_p of N = 2B points, is run on a reference x and adapted
 * so that its output y follows a desired signal d.  Each call takes B samples of x
 * and d per channel and writes the B samples of the error e = d - y (and of y when
 * asked): echo and feedback cancellation, system identification, noise cancellation
 * with a reference.  The latency is B samples and every call emits.  Supported
 * blocks: B in {128, 256, 512, 1024} (crlot_stream_convolve_hop's register-resident
 * transforms; the B = 1024 instantiation builds without scratch); any other block a
 * plan accepts is CRLOT_EUNSUPPORTED; a block no plan accepts is CRLOT_EINVAL.
 *
 * Values.  float32 throughout; per channel and hop k, counted from create / reset:
 *   1  xb = sanitize(x block) (x = NULL: zeros), db = sanitize(d block);
 *   2  the frame [prev, xb], no window; X_k = the per-frame forward transform and
 *      kiss_fftr split, stored in row k mod P of a ring of P spectrum rows; then prev =
 *      xb.  X_k equals, bit for bit, row k of crlot_stft with frame pairing off on a
 *      plan with frame N = 2B, hop B and a window of ones, over the reference prefixed
 *      by B zeros (= crlot_rfft_batched of the frame on that plan);
 *   3  Y from re = im = +0, for j = max(0, k-P+1) .. k ascending, p = k - j: the
 *      streaming convolver's four fmaf with H := W_p and X_j, then + 0.0f.  Rows of
 *      hops that have not happened are not read;
 *   4  o = sanitize(inverse(kiss_fftri merge(Y)) * 1/N); y = o[B .. 2B); e = db - y, one
 *      subtraction; e is stored, y when d_y is not NULL;
 *   5  adapting: E = the forward transform and split of the frame [+0 x B, e], sanitized
 *      as every forward entry sanitizes its input (= crlot_rfft_batched of that frame);
 *   6  per bin: m = (Xr Xr) + (Xi Xi); pw = m at k = 0, else (lambda pw) + (omega m),
 *      whether adapting or not.  Adapting: g = mu_P / (pw + delta), G = (g Er, g Ei).
 *      Every product, sum and quotient is rounded on its own (no FMA), the division
 *      correctly rounded;
 *   7  adapting, every p with k - p >= 0 and every bin, X = ring row (k - p) mod P:
 *        re = fmaf(Xr, Gr, Wr); re = fmaf(Xi, Gi, re);
 *        im = fmaf(Xr, Gi, Wi); im = fmaf(-Xi, Gr, im);     (W_p += conj(X) G)
 *   8  adapting, the gradient constraint on partition k mod P (mode 1) or on every
 *      partition (mode 2): w = inverse(merge(W_p)) * 1/N; w[B .. 2B) = +0; W_p = forward
 *      and split of w (no sanitize in either direction).
 * The constants are set by crlot_fdaf_set_step(mu, lambda, delta), defaults 0.5, 0.9,
 * 1e-3: mu_P = float32(mu / P) and omega = float32(1 - lambda), both formed in double,
 * lambda and delta rounded to float32 (CRLOT_EINVAL unless 0 <= mu <= 2, 0 <= lambda < 1,
 * delta > 0, all finite).  crlot_fdaf_set_constraint: 0 none, 1 round-robin (default),
 * 2 every partition every hop.  crlot_fdaf_set_adapt(af, 0) freezes the filter: steps
 * 1 - 4 and the power estimate of step 6 alone.  The bits of e, y and the state never
 * depend on the channel count, a channel's position, the layout or the constraint
 * kernel's grid: mode 1 equals mode 0 hops each followed by crlot_fdaf_constrain(af,
 * k mod P), mode 2 equals mode 0 hops each followed by crlot_fdaf_constrain(af, -1).
 *
 * Kernels.  A hop enqueues, on the caller's stream, CRLOT_K_FDAF_HOP (steps 1 - 6, one
 * wave per channel; e and y are complete after it), then when adapting
 * CRLOT_K_FDAF_UPDATE (step 7, one wave per 64 bins of a channel) and, in modes 1 and
 * 2, CRLOT_K_FDAF_CONSTRAIN (step 8, one wave per channel and partition).
 * crlot_fdaf_last_launch lists the last hop's.  crlot_fdaf_constrain(af, p, stream)
 * runs step 8 alone on partition p of every channel, or on all partitions with p = -1
 * (CRLOT_EINVAL: p outside -1 .. P-1).
 *
 * Taps.  crlot_fdaf_set_taps(af, h, n_rows, ld) loads K taps per channel from host
 * rows ld >= K floats apart (n_rows = channels, or 1: one row for every channel;
 * CRLOT_EINVAL otherwise or for a tap that is not finite): W_p = crlot_rfft_batched of
 * partition p zero-padded to N on the internal plan, as a crlot_convolver's spectra.
 * crlot_fdaf_get_taps(af, out, ld) writes K floats per channel: the first B samples of
 * crlot_irfft_batched of each W_p, partition after partition.  Both synchronise the
 * device.  crlot_fdaf_state returns the device pointers of the state (any may be NULL):
 * per channel ring [P][N+2], W [P][N+2], pw [B+1], E [N+2], G [N+2], prev [B], floats,
 * channels adjacent.
 *
 * crlot_fdaf_create touches no device (CRLOT_EINVAL: a null out, a block no plan
 * accepts, K < 1 or K > 2^20, channels < 1, a state size or grid that does not fit).
 * crlot_fdaf_prepare, or the first call that needs the device, makes the internal plan
 * (frame 2B, hop B) on the current device and allocates and zeroes the state
 * (crlot_fdaf_state_bytes, valid before prepare; CRLOT_ENOMEM when it does not fit).
 * A single-owner object like crlot_stream: the hops of one object go on one stream or
 * are ordered by the caller.  Graph capture is not supported (the hop index is a
 * by-value kernel argument).  Blocks are channel-major [channels][B], or [B][channels]
 * after crlot_fdaf_set_layout(af, 1), for x, d, e and y alike.  crlot_fdaf_reset
 * synchronises the device and zeroes the state (the weights too) and the hop counter.
 * crlot_fdaf_hop: CRLOT_EINVAL for a null af, d_d or d_e, or when an output block
 * overlaps an input block or the other output. */
typedef struct crlot_fdaf crlot_fdaf;
typedef struct crlot_fdaf_launch {
    int32_t hop_kernel;        /* CRLOT_K_FDAF_HOP; 0: no hop yet */
    int32_t update_kernel;     /* CRLOT_K_FDAF_UPDATE; 0: the last hop did not adapt */
    int32_t constrain_kernel;  /* CRLOT_K_FDAF_CONSTRAIN; 0: mode 0 or not adapting */
    int32_t reserved;
    int64_t hop_grid;          /* workgroups: ceil(channels / 4) */
    int64_t update_grid;       /* workgroups: channels * ceil((B + 1) / 64) */
    int64_t constrain_grid;    /* workgroups: ceil(channels * partitions constrained / 4) */
} crlot_fdaf_launch;
int crlot_fdaf_create(int32_t block, int64_t taps, int32_t channels, crlot_fdaf** out);
void crlot_fdaf_destroy(crlot_fdaf* af);
int crlot_fdaf_prepare(crlot_fdaf* af);
int64_t crlot_fdaf_state_bytes(const crlot_fdaf* af);
int crlot_fdaf_reset(crlot_fdaf* af);
int crlot_fdaf_set_layout(crlot_fdaf* af, int32_t interleaved);
int crlot_fdaf_info(const crlot_fdaf* af, int32_t* channels, int32_t* block, int64_t* taps, int32_t* P,
                    int64_t* hops);
int crlot_fdaf_last_launch(const crlot_fdaf* af, crlot_fdaf_launch* out);
int crlot_fdaf_set_step(crlot_fdaf* af, double mu, double lambda, double delta);
int crlot_fdaf_set_constraint(crlot_fdaf* af, int32_t mode /* 0 none, 1 round-robin, 2 all */);
int crlot_fdaf_set_adapt(crlot_fdaf* af, int32_t on /* default 1 */);
int crlot_fdaf_set_taps(crlot_fdaf* af, const float* h /* host [n_rows][ld] */, int32_t n_rows, int64_t ld);
int crlot_fdaf_get_taps(crlot_fdaf* af, float* host_out /* [channels][ld] */, int64_t ld);
int crlot_fdaf_state(crlot_fdaf* af, float** ring, float** W, float** pw, float** E, float** G, float** prev);
int crlot_fdaf_hop(crlot_fdaf* af, const float* d_x /* NULL: zeros */, const float* d_d, float* d_e,
                   float* d_y /* may be NULL */, void* stream);
int crlot_fdaf_constrain(crlot_fdaf* af, int32_t p /* -1: all */, void* stream);

/* ---------------------------------------------------------------- noise suppressor
 * A stationary-noise suppressor on the spectral step: MCRA noise tracking (Cohen &
 * Berdugo 2002, without its smoothing along frequency) and a decision-directed Wiener
 * gain (Ephraim & Malah 1984).  Per (channel, bin b <= N/2) six float32 state values --
 * S, Smin, Stmp, p, lam, A2 -- are carried from frame to frame; frame k's gain row G
 * [N/2+1] is what crlot_plan_set_spectral_mask / crlot_stream_push_hop_masked take as a
 * mask row.  Offline: crlot_denoise_gains (spectra -> mask rows) and crlot_denoise
 * (x -> y).  Per hop: crlot_stream_denoise_hop, the state inside the hop's launch.
 *
 * Values.  float32, every product, sum and quotient rounded on its own (no FMA), the
 * division correctly rounded; min(a, b) is a < b ? a : b and max(a, b) is a > b ? a : b.
 * Each factor alpha_* of the descriptor is rounded to float32 and its complement is
 * omega_* = float32(1 - alpha_*), formed in double.  X is the row crlot_stft /
 * crlot_stream_stft_hop stores for the frame: before the plan gain, the DC and Nyquist
 * imaginary parts 0.  Per bin and frame k, counted from create / reset (or k0 + row):
 *   1  P = (Xr Xr) + (Xi Xi);
 *   2  k = 0: S = Smin = Stmp = lam = P, p = 0, A2 = 0;
 *   3  k > 0: S = (alpha_s S) + (omega_s P);
 *      k mod window == 0: Smin = min(Stmp, S), Stmp = S;
 *      otherwise:         Smin = min(Smin, S), Stmp = min(Stmp, S);
 *      I = S > (delta Smin);  p = (alpha_p p) + (I ? omega_p : 0);
 *      ad = alpha_d + (omega_d p);  lam = (ad lam) + ((1 - ad) P);
 *   4  lc = max(lam, 1e-30f); gamma = P / lc;
 *      xi = (alpha_dd (A2 / lc)) + (omega_dd max(gamma - 1, 0));
 *   5  G = max(xi / (1 + xi), g_min);  A2 = (G G) P;
 *   6  the step on the frame is ((X gain) G) on re and im each: a mask row G.
 * Output bits do not depend on the grid, the stream count, the leading dimensions, a
 * channel's position, or where a run is cut: the gains of F frames equal the gains of F1
 * frames followed by those of F - F1 with the state carried.
 *
 * Descriptor (crlot_denoise_desc_default fills the defaults): alpha_s 0.8, alpha_p 0.2,
 * alpha_d 0.95, alpha_dd 0.98, each in [0, 1); delta 5 (> 0); window 64 frames (>= 1);
 * g_min 0.1 in [0, 1].  It is checked before any device work: a value outside its range
 * or not finite is CRLOT_EINVAL.
 *
 * crlot_denoiser_create(plan, desc, channels, out) touches no device (CRLOT_EINVAL: a null
 * argument, a bad descriptor, channels < 1, a state size or grid that does not fit).  prepare, or
 * the first call that needs it, allocates the state block [channels][6][N/2+1] (planes in
 * the order above), one spectrum row and one mask row per channel (the staged hop's), zeroed.
 * crlot_denoiser_state returns the state block's device pointer; crlot_denoiser_reset
 * synchronises the device, zeroes the block and the frame counter.  A single-owner object
 * like crlot_stream; graph capture is not supported (the frame index is by value).
 *
 * crlot_denoise_gains(dn, d_spec, d_mask, n_streams, F, ld_spec, ldf_spec, ld_mask, ldf_mask,
 * carry, stream): spectra in crlot_stft's layout (frame f of stream s at d_spec + s ld_spec
 * + f ldf_spec, N/2+1 float pairs, 8-byte aligned, even leading dimensions) -> mask rows
 * (d_mask + s ld_mask + f ldf_mask, N/2+1 floats).  carry = 0: every stream starts at
 * frame 0 with fresh state kept in registers; the object's state is neither read nor
 * written, any n_streams.  carry = 1: n_streams must equal the channel count; the run
 * continues from the object's state and frame counter and advances both.  One launch,
 * CRLOT_K_DENOISE_GAINS: a lane per (stream, bin) column walks the frames in order (the
 * recurrence is not linear, so a column is not chunked), adjacent lanes adjacent bins.
 * n_streams or F of 0: CRLOT_OK, nothing written.  CRLOT_EINVAL: null buffers, a leading
 * dimension too small or odd where pairs need it even, a mask that overlaps the spectra.
 *
 * crlot_denoise(dn, d_x, d_y, n_streams, T, ld_x, ld_y, stream) = crlot_stft -> the gains
 * (carry = 0) -> crlot_istft_ola with the gains as the per-frame mask, spectra and gains
 * in the stream's sliced workspace (slices under 256 MiB or one stream's worth); bit for
 * bit the hand composition under either frame-pairing setting.  The mask is passed to the
 * synthesis half as an argument, as crlot_hpss passes its masks: nothing is stored in the
 * plan, and a plan that holds a stored mask of its own is CRLOT_EINVAL.  y gets F H
 * samples per stream, F = crlot_frame_count(T).
 *
 * crlot_stream_denoise_hop(st, dn, d_hop_in, d_hop_out, emitted, stream): push_hop with
 * frame k's gain row, computed from frame k's own spectrum, as the mask of the frame the
 * hop completes.  A whole-mode call (it mixes with push_hop / push_hop_masked as far as
 * the frame counters allow); a hop that completes no frame touches no state.  The frame
 * index is the stream's.  CRLOT_EINVAL: a null argument, dn created on another plan,
 * another channel count.  CRLOT_ERUNTIME: dn's frame counter differs from the frames the
 * stream has completed (until both are reset), or the stream is in split mode.  Routes
 * (crlot_denoiser_set_route: 0 the library's choice, 1 fused, 2 staged; CRLOT_EUNSUPPORTED
 * for 1 at a shape without the fused kernel):
 *   fused   one launch, CRLOT_K_DENOISE_HOP: the state planes of the lane's bins are read
 *           where push_hop_masked reads its mask row, advanced between split and merge,
 *           stored back; no spectrum in HBM.  Shapes: the register-resident hop's with
 *           N <= 1024.  The library's choice there.
 *   staged  three launches: the analysis half (CRLOT_K_STREAM_STFT) into the object's
 *           spectrum rows, CRLOT_K_DENOISE_GAINS with F = 1 on the object's state, the
 *           synthesis half (CRLOT_K_STREAM_ISTFT) with the gains as its mask row.  Every
 *           other shape a stream accepts, N = 2048 and the mixed-radix ones included.
 * Both routes give the same bits, equal to crlot_denoise's over the concatenated hops
 * with frame pairing off in DROP mode.  crlot_denoiser_last_launch lists the last hop's
 * (or the last crlot_denoise_gains call's) kernels and grids. */
typedef struct crlot_denoiser crlot_denoiser;
typedef struct crlot_denoise_desc {
    double alpha_s;   /* smoothing of the power S along time */
    double alpha_p;   /* smoothing of the speech-presence probability p */
    double alpha_d;   /* floor of the noise estimate's smoothing factor */
    double delta;     /* presence threshold on S / Smin */
    double alpha_dd;  /* decision-directed weight of the a-priori SNR */
    double g_min;     /* gain floor */
    int32_t window;   /* minimum-tracking window L, frames */
    int32_t reserved;
} crlot_denoise_desc;
typedef struct crlot_denoise_launch {
    int32_t route;      /* 1 fused, 2 staged (hops); 0: the last call was crlot_denoise_gains, or none yet */
    int32_t n_kernels;  /* 0: no launch yet; 1: gains, a fused hop, or a staged hop that completed no frame; 3: a staged hop */
    int32_t kernel[3];  /* CRLOT_K_* in launch order */
    int32_t reserved;
    int64_t grid[3];    /* workgroups of each (0 for a mixed-radix hop half: its launcher sizes the workgroups) */
} crlot_denoise_launch;
int crlot_denoise_desc_default(crlot_denoise_desc* desc);
int crlot_denoiser_create(crlot_plan* plan, const crlot_denoise_desc* desc, int32_t channels, crlot_denoiser** out);
void crlot_denoiser_destroy(crlot_denoiser* dn);
int crlot_denoiser_prepare(crlot_denoiser* dn);
int crlot_denoiser_reset(crlot_denoiser* dn);
int crlot_denoiser_info(const crlot_denoiser* dn, int32_t* channels, int32_t* bins, int64_t* frames,
                        int32_t* route /* the setter's value */, int32_t* fused_ok);
int crlot_denoiser_state(crlot_denoiser* dn, float** d_state /* [channels][6][N/2+1] */);
int crlot_denoiser_set_route(crlot_denoiser* dn, int32_t route /* 0 auto, 1 fused, 2 staged */);
int crlot_denoiser_last_launch(const crlot_denoiser* dn, crlot_denoise_launch* out);
int crlot_denoise_gains(crlot_denoiser* dn, const float* d_spec, float* d_mask, int32_t n_streams, int64_t F,
                        int64_t ld_spec, int64_t ldf_spec, int64_t ld_mask, int64_t ldf_mask, int32_t carry,
                        void* stream);
int crlot_denoise(crlot_denoiser* dn, const float* d_x, float* d_y, int32_t n_streams, int64_t T, int64_t ld_x,
                  int64_t ld_y, void* stream);
int crlot_stream_denoise_hop(crlot_stream* st, crlot_denoiser* dn, const float* d_hop_in, float* d_hop_out,
                             int32_t* emitted, void* stream);

/* ---------------------------------------------------------------- cross-spectral estimation
 * Averaged auto- and cross-spectra of two signals along the frame axis of crlot_stft's
 * spectra, and what a voice chain derives from them: the magnitude-squared coherence (the
 * double-talk / "is this reference useful" statistic), the H1 transfer-function estimate
 * Sab / Saa (what crlot_fdaf converges to: a warm start for crlot_fdaf_set_taps), and the
 * GCC-PHAT estimate of the bulk delay of b against a.  Per (pair, bin b <= N/2) four
 * float32 values -- Saa, Sbb, Sr, Si -- are carried from frame to frame.
 *
 * Values.  float32, every product, sum, difference and quotient rounded on its own (no
 * FMA), division and sqrtf correctly rounded; max(a, b) is a > b ? a : b.  A (reference)
 * and B (desired) are rows crlot_stft / crlot_stream_stft_hop store: before the plan gain.
 * State: a block [pair][4][N/2+1] in the order Saa, Sbb, Sr, Si, all 0 after create / reset.
 *   1  terms of frame k:  Taa = (ar ar) + (ai ai);  Tbb = (br br) + (bi bi);
 *      Tr = (ar br) + (ai bi);  Ti = (ar bi) - (ai br)          -- conj(A) B, as scipy's
 *      csd(x, y): H1 is the transfer function from a to b, and b delayed against a gives
 *      a positive lag;
 *   2  each plane S = (lambda S) + (omega T).  alpha = 0 (Welch): lambda = omega = 1, both
 *      products exact, the planes are plain sums in frame order (the mean is the caller's
 *      division by the frame count; nothing below needs it).  alpha in (0, 1): lambda =
 *      float32(alpha), omega = float32(1 - alpha) formed in double.  No first-frame case:
 *      from zero state (lambda 0) + (omega T) is omega T;
 *   3  rows derived from a state block, tiny = 1e-30f, m2 = (Sr Sr) + (Si Si):
 *      coherence C = m2 / max(Saa Sbb, tiny), not clamped to 1;
 *      transfer  d = max(Saa, tiny), H1 = (Sr / d, Si / d), a spectrum row of N/2+1 float
 *        pairs (what crlot_irfft_batched takes);
 *      weighted cross-spectrum W, a spectrum row: weighting 0: (Sr, Si); weighting 1 (PHAT):
 *        m = sqrtf(m2), e = max(m, tiny), W = (Sr / e, Si / e);
 *   4  peak of a row cc[n], n < N, over max_lag in [1, N/2 - 1]: position j = 0 .. 2 max_lag
 *      is lag l = j - max_lag with value v_j = cc[l mod N].  The winner starts as j = 0; a
 *      later j replaces it only if v_j > the best value so far: the smallest j among equal
 *      maxima wins and a NaN at j > 0 never wins (a NaN at j = 0 is never replaced: nothing
 *      compares greater).  With y0, y1, y2 = cc at l - 1, l, l + 1 (mod N): den = (y0 -
 *      (2 y1)) + y2, frac = den == 0 ? 0 : (0.5 (y0 - y2)) / den.  Output row per pair:
 *      three floats {float(l), frac, y1}; the delay in samples is the sum of the first two.
 * Output bits do not depend on the grid, the pair count, the leading dimensions, a pair's
 * position, a shared or a repeated reference, or where a run is cut: F frames equal F1
 * frames followed by F - F1 with the state carried.
 *
 * crlot_xspec_create(plan, n_pairs, alpha, out) touches no device.  alpha is checked first:
 * NaN, Inf, < 0 or >= 1 is CRLOT_EINVAL with no plan needed; then a null argument, n_pairs
 * < 1, a state size or grid that does not fit.  prepare, or the first call that needs it,
 * makes one allocation: the state block, zeroed.  crlot_xspec_state returns its device
 * pointer; crlot_xspec_reset synchronises the device, zeroes the block and the frame
 * counter.  A single-owner object like crlot_stream; graph capture is not supported (the
 * frame counter is by value).
 *
 * crlot_xspec_accumulate(xs, d_a, d_b, n_pairs, F, ld_a, ldf_a, ld_b, ldf_b, carry,
 * d_state_out, stream): spectra in crlot_stft's layout (frame f of pair p at d + p ld +
 * f ldf, N/2+1 float pairs, 8-byte aligned, even leading dimensions); ld_a = 0: one
 * reference stream shared by every pair, as a mask's ld_stream = 0.  carry = 0: every pair
 * starts from zero state kept in registers, any n_pairs, the result goes to d_state_out
 * (required, [n_pairs][4][N/2+1]), the object is untouched.  carry = 1: n_pairs must equal
 * the object's; the run continues from the object's state and counter and advances both;
 * d_state_out may be NULL (else it receives a copy of the new state).  One launch,
 * CRLOT_K_XSPEC_ACC: a lane per (pair, bin) column walks the frames in order.  F = 1 with
 * carry = 1 on the rows of two crlot_stream_stft_hop streams is the per-hop tracker.
 * n_pairs or F of 0: CRLOT_OK, nothing written.  CRLOT_EINVAL: null buffers, a leading
 * dimension too small or odd, a state output that overlaps an input.
 *
 * crlot_xspec_derive(xs, d_state, n_pairs, weighting, d_coh, ld_coh, d_h1, ld_h1, d_w, ld_w,
 * stream): d_state NULL: the object's state (n_pairs must equal the object's).  Any
 * non-empty subset of the three outputs in one pass (CRLOT_K_XSPEC_DERIVE); row p at d +
 * p ld: coherence N/2+1 floats, H1 and W N/2+1 float pairs (8-byte aligned, even ld).
 * CRLOT_EINVAL: no output, weighting outside 0 / 1, a leading dimension too small or odd,
 * outputs that overlap each other or the state.
 *
 * crlot_xspec_peak(xs, d_cc, ld_cc, n_pairs, max_lag, d_out, ld_out, stream): step 4 on
 * caller rows of N floats (CRLOT_K_XSPEC_PEAK, a wave per pair); ld_out >= 3.  Lags are
 * limited to +-(N/2 - 1) of the plan's frame: a longer search takes a plan with a longer
 * frame.
 *
 * crlot_xspec_estimate(xs, d_xa, d_xb, n_pairs, T, ld_xa, ld_xb, carry, d_state_out,
 * stream) = crlot_stft(a) -> crlot_stft(b) -> accumulate over F = crlot_frame_count(T)
 * frames; ld_xa = 0: a shared reference (one transform of it).  The spectra stay in the
 * stream's sliced workspace (slices of pairs under 256 MiB or one pair's worth); bit for
 * bit the hand composition under either frame-pairing setting.
 *
 * crlot_xspec_delay(xs, d_state, n_pairs, weighting, max_lag, d_out, ld_out, stream) =
 * derive(W) -> crlot_irfft_batched on the object's plan -> peak, W and cc in the stream's
 * scratch; every N crlot_irfft_batched accepts on that plan; bit for bit the hand
 * composition.  crlot_xspec_last_launch lists the last call's kernels of this subsystem
 * and their grids (the transforms of estimate and delay are in crlot_plan_last_launch). */
typedef struct crlot_xspec crlot_xspec;
typedef struct crlot_xspec_launch {
    int32_t n_kernels;    /* 0: no launch yet */
    int32_t kernel[3];    /* CRLOT_K_* in launch order */
    int32_t reserved[2];
    int64_t grid[3];      /* workgroups of each */
} crlot_xspec_launch;
int crlot_xspec_create(crlot_plan* plan, int32_t n_pairs, double alpha, crlot_xspec** out);
void crlot_xspec_destroy(crlot_xspec* xs);
int crlot_xspec_prepare(crlot_xspec* xs);
int crlot_xspec_reset(crlot_xspec* xs);
int crlot_xspec_info(const crlot_xspec* xs, int32_t* pairs, int32_t* bins, int64_t* frames, float* lambda,
                     float* omega);
int crlot_xspec_state(crlot_xspec* xs, float** d_state /* [pairs][4][N/2+1] */);
int crlot_xspec_last_launch(const crlot_xspec* xs, crlot_xspec_launch* out);
int crlot_xspec_accumulate(crlot_xspec* xs, const float* d_a, const float* d_b, int32_t n_pairs, int64_t F,
                           int64_t ld_a /* 0: shared */, int64_t ldf_a, int64_t ld_b, int64_t ldf_b, int32_t carry,
                           float* d_state_out /* carry = 1: may be NULL */, void* stream);
int crlot_xspec_derive(crlot_xspec* xs, const float* d_state /* NULL: the object's */, int32_t n_pairs,
                       int32_t weighting /* 0 none, 1 PHAT */, float* d_coh, int64_t ld_coh, float* d_h1,
                       int64_t ld_h1, float* d_w, int64_t ld_w, void* stream);
int crlot_xspec_peak(crlot_xspec* xs, const float* d_cc, int64_t ld_cc, int32_t n_pairs, int32_t max_lag,
                     float* d_out /* [n_pairs][ld_out >= 3] */, int64_t ld_out, void* stream);
int crlot_xspec_estimate(crlot_xspec* xs, const float* d_xa, const float* d_xb, int32_t n_pairs, int64_t T,
                         int64_t ld_xa /* 0: shared */, int64_t ld_xb, int32_t carry, float* d_state_out,
                         void* stream);
int crlot_xspec_delay(crlot_xspec* xs, const float* d_state /* NULL: the object's */, int32_t n_pairs,
                      int32_t weighting, int32_t max_lag, float* d_out, int64_t ld_out, void* stream);

/* ---------------------------------------------------------------- beamformer
 * A mask-driven frequency-domain MVDR beamformer: G independent groups (arrays) of M
 * microphones, 2 <= M <= 8, combined into one output stream per group.  The inputs are what
 * the library already makes -- spectra in crlot_stft's layout, mask rows such as
 * crlot_denoise_gains', inter-microphone delays from crlot_xspec_delay (as a steering
 * vector) -- and the output is a spectrum row for crlot_istft_ola / crlot_stream_istft_hop.
 * The reference project has no beamformer: nothing in this section restates it, and no
 * entry below cites it.
 *
 * Terms.  Stream g M + m is microphone m of group g: frame f of stream s at d_spec + s
 * ld_spec + f ldf_spec, N/2+1 float pairs, as crlot_stft / crlot_stream_stft_hop store them
 * (before the plan gain).  ref is the reference microphone, 0 <= ref < M.
 *
 * Values.  float32, every product, sum, difference and quotient rounded on its own (no
 * FMA), division and sqrtf correctly rounded; max(a, b) is a > b ? a : b; tiny = 1e-30f.
 * Complex products, each product rounded before the sum or difference:
 *   a conj(b) = ((a.re b.re) + (a.im b.im), (a.im b.re) - (a.re b.im))
 *   conj(a) b = ((a.re b.re) + (a.im b.im), (a.re b.im) - (a.im b.re))
 *   a b       = ((a.re b.re) - (a.im b.im), (a.re b.im) + (a.im b.re))
 * and a complex value is subtracted, added or divided by a real per component.
 * State: per (group, bin b <= N/2) two Hermitian matrices, Phi_s (target) then Phi_n
 * (noise), each M M float planes: the M real diagonals Phi_00 .. Phi_{M-1,M-1}, then for
 * every i < j in lexicographic order Re Phi_ij, Im Phi_ij.  The block is
 * [group][2][M M][N/2+1], all 0 after create / reset.
 *   1  terms of frame k, Phi_ij averaging x_i conj(x_j): diagonal T = (re re) + (im im);
 *      i < j: T = x_i conj(x_j) as above;
 *   2  update.  mu is the mask value of (group, frame, bin), 1 without a mask; nu = 1 - mu.
 *      target 0: Phi_s with weight mu and Phi_n with weight nu (a mask is required);
 *      target 1: Phi_s alone, weight mu;  target 2: Phi_n alone, weight mu (calibration on a
 *      noise-only stretch).  Each plane S = (lambda S) + (omega (wgt T)); lambda and omega
 *      from alpha as crlot_xspec forms them (alpha = 0: 1 and 1, Welch sums; alpha in (0, 1):
 *      float32(alpha), float32(1 - alpha) formed in double).  No first-frame case;
 *   3  solve per (group, bin).  tr = Phi_n00, then + Phi_n11 ... in index order; ld =
 *      max(loading_f32 (tr / float(M)), tiny); A_ii = Phi_nii + ld, A_ij = Phi_nij.
 *      Cholesky A = L L^H, j ascending: s = A_jj, then for k < j ascending s = s -
 *      ((L_jk.re L_jk.re) + (L_jk.im L_jk.im)); d_j = sqrtf(max(s, tiny)); for i > j:
 *      c = A_ij = conj(A_ji), then for k < j ascending c = c - L_ik conj(L_jk); L_ij = c / d_j.
 *      Forward L z = r: i ascending, t = r_i, for k < i ascending t = t - L_ik z_k, z_i =
 *      t / d_i.  Back L^H y = z: i descending, t = z_i, for k > i ascending t = t -
 *      conj(L_ki) y_k, y_i = t / d_i.
 *      mode 0 (SOUDEN; Souden, Benesty, Affes 2010): solve for every column c of Phi_s (read
 *      from the Hermitian storage, the lower part the conjugate, the diagonal's imaginary
 *      part 0); trace = Re y(0)_0, then + Re y(c)_c in c order; den = max(trace, tiny); w =
 *      y(ref) / den.
 *      mode 1 (STEERED, the classical MVDR): r = d, the steering vector of the bin
 *      ([group][M][N/2+1] float pairs); q = (d_0.re y_0.re) + (d_0.im y_0.im), then + the
 *      same of m = 1 .. in m order; den = max(q, tiny); w = y / den.  Only Phi_n is read.
 *      Weights are a block [group][M][N/2+1] float pairs; after create / reset (1, 0) at
 *      ref and 0 elsewhere, which passes the reference microphone through;
 *   4  apply.  Y = sum over m ascending of conj(w_m) x_m, accumulated per component from
 *      (0, 0), stored as N/2+1 float pairs.  The imaginary parts of DC and Nyquist are
 *      stored as computed; crlot_istft_ola and crlot_stream_istft_hop ignore them.
 * Output bits do not depend on the grid, the group count, a group's position, the leading
 * dimensions, a shared or a repeated mask, where a run is cut (F frames equal F1 frames
 * followed by F - F1 with the state carried), or how the matrix entries are spread over
 * lanes.
 *
 * crlot_beamformer_create(plan, desc, groups, out) touches no device.  The descriptor is
 * checked first, with no plan needed: mics outside 2..8, ref outside 0..mics-1, mode
 * outside 0 / 1, update_every < 1, alpha NaN / Inf / < 0 / >= 1, loading NaN / Inf / < 0 are
 * CRLOT_EINVAL; then a null argument, groups < 1, a size or grid that does not fit.
 * prepare, or the first call that needs it, makes one allocation: the state, the weights
 * (set to pass ref through), the steering block (zero) and the rows of the per-hop entry.
 * _state, _weights and _steering return device pointers the caller may read and write
 * (crlot_beamformer_steering is how a STEERED object gets its vectors); _reset synchronises
 * the device, zeroes the state, restores the pass-through weights and zeroes the frame
 * counter (the steering block is kept).  A single-owner object like crlot_stream; graph
 * capture is not supported (the frame counter is by value).
 *
 * crlot_beamform_accumulate(bf, d_spec, ld_spec, ldf_spec, d_mask, ld_mask, ldf_mask,
 * n_groups, F, target, carry, d_state_out, stream): steps 1 and 2 over F frames of n_groups
 * M streams (CRLOT_K_BF_ACC).  The mask value of group g, frame f, bin b is d_mask[g ld_mask
 * + f ldf_mask + b]; ld_mask = 0: one set of rows shared by every group; d_mask NULL: 1
 * (targets 1 and 2).  carry = 0: every group starts from zero state kept in registers, any
 * n_groups, the result goes to d_state_out (required), the object is untouched; a matrix
 * the target does not update is not written.  carry = 1: n_groups must equal the
 * object's; the run continues from the object's state and counter and advances both;
 * d_state_out may be NULL (else it receives a copy of the new state).  n_groups or F of 0:
 * CRLOT_OK, nothing written.  CRLOT_EINVAL: null buffers, a leading dimension too small or
 * (spectra) odd, target outside 0..2 or 0 without a mask, a state output that overlaps an
 * input or the object's state.
 *
 * crlot_beamform_solve(bf, d_state, d_steer, n_groups, d_w, stream): step 3 in the
 * object's mode (CRLOT_K_BF_SOLVE); NULL for a block means the object's (then n_groups must
 * equal the object's).  crlot_beamform_apply(bf, d_spec, ld_spec, ldf_spec, d_w, n_groups,
 * F, d_out, ld_out, ldf_out, stream): step 4 (CRLOT_K_BF_APPLY), frame f of group g at d_out
 * + g ld_out + f ldf_out.  CRLOT_EINVAL: outputs that overlap an input, the state or the
 * weights.
 *
 * crlot_beamform(bf, d_x, ld_x, d_mask, ld_mask, ldf_mask, d_y, ld_y, n_groups, T, stream) =
 * crlot_stft of the n_groups M signals (stream s at d_x + s ld_x) -> accumulate (carry = 0,
 * target 0) -> solve -> apply -> crlot_istft_ola of the n_groups outputs (group g at d_y +
 * g ld_y, F H samples).  In STEERED mode d_mask may be NULL: Phi_n is then accumulated from
 * every frame with weight 1 (target 2), the "minimum power" MPDR form, which cancels the
 * target too wherever the steering vector is off.  Everything between stays in the
 * stream's sliced workspace, sliced by group (slices under 256 MiB or one group's worth);
 * bit for bit the hand composition under either frame-pairing setting.  The object's
 * state, weights and counter are untouched (its steering block is read).  A plan that
 * holds a stored spectral mask is CRLOT_EINVAL, as for crlot_denoise.
 *
 * crlot_stream_beamform_hop(st_in, st_out, bf, d_hop_in, d_mask, ld_mask, d_hop_out,
 * emitted, stream): one hop of the per-hop chain.  st_in has groups M channels and uses
 * only its analysis half, st_out has groups channels and only its synthesis half; both in
 * split mode on bf's plan.  A hop = crlot_stream_stft_hop into the object's rows ->
 * CRLOT_K_BF_HOP -> crlot_stream_istft_hop: three launches, bit for bit stft_hop ->
 * accumulate(F = 1, carry = 1, target 0) -> solve when due -> apply(F = 1) -> istft_hop.
 * d_mask is the frame's mask row per group (ld_mask 0: shared), required.  The solve runs
 * when (frames so far + 1) mod update_every == 0, after the update and before the apply.
 * A hop that completes no frame runs only the analysis half, leaves d_hop_out untouched
 * and sets *emitted = 0 (else the hop size).  CRLOT_EINVAL: channel counts or plans that do
 * not match; CRLOT_ERUNTIME: frame counters that differ (reset all three), a stream in
 * whole-hop mode.  crlot_beamformer_last_launch lists the last call's kernels and grids. */
#define CRLOT_BF_SOUDEN 0
#define CRLOT_BF_STEERED 1
typedef struct crlot_beamform_desc {
    int32_t mics;          /* M, 2..8 */
    int32_t ref;           /* the reference microphone */
    int32_t mode;          /* CRLOT_BF_SOUDEN, CRLOT_BF_STEERED */
    int32_t update_every;  /* >= 1: hops between the per-hop entry's solves */
    double alpha;          /* [0, 1): 0 Welch sums, else exponential averaging */
    double loading;        /* >= 0, finite: diagonal loading relative to trace / M (default 1e-3) */
} crlot_beamform_desc;
typedef struct crlot_beamformer crlot_beamformer;
typedef struct crlot_beamform_launch {
    int32_t n_kernels;    /* 0: no launch yet */
    int32_t kernel[3];    /* CRLOT_K_* in launch order */
    int32_t reserved[2];
    int64_t grid[3];      /* workgroups of each */
} crlot_beamform_launch;
int crlot_beamform_desc_default(crlot_beamform_desc* d);
int crlot_beamformer_create(crlot_plan* plan, const crlot_beamform_desc* desc, int32_t groups, crlot_beamformer** out);
void crlot_beamformer_destroy(crlot_beamformer* bf);
int crlot_beamformer_prepare(crlot_beamformer* bf);
int crlot_beamformer_reset(crlot_beamformer* bf);
int crlot_beamformer_info(const crlot_beamformer* bf, int32_t* groups, int32_t* mics, int32_t* bins, int64_t* frames,
                          float* lambda, float* omega, float* loading);
int crlot_beamformer_state(crlot_beamformer* bf, float** d_state /* [groups][2][M M][N/2+1] */);
int crlot_beamformer_weights(crlot_beamformer* bf, float** d_w /* [groups][M][N/2+1] float pairs */);
int crlot_beamformer_steering(crlot_beamformer* bf, float** d_steer /* [groups][M][N/2+1] float pairs */);
int crlot_beamformer_last_launch(const crlot_beamformer* bf, crlot_beamform_launch* out);
int crlot_beamform_accumulate(crlot_beamformer* bf, const float* d_spec, int64_t ld_spec, int64_t ldf_spec,
                              const float* d_mask, int64_t ld_mask /* 0: shared */, int64_t ldf_mask, int32_t n_groups,
                              int64_t F, int32_t target, int32_t carry, float* d_state_out /* carry = 1: may be NULL */,
                              void* stream);
int crlot_beamform_solve(crlot_beamformer* bf, const float* d_state /* NULL: the object's */,
                         const float* d_steer /* NULL: the object's */, int32_t n_groups,
                         float* d_w /* NULL: the object's */, void* stream);
int crlot_beamform_apply(crlot_beamformer* bf, const float* d_spec, int64_t ld_spec, int64_t ldf_spec,
                         const float* d_w /* NULL: the object's */, int32_t n_groups, int64_t F, float* d_out,
                         int64_t ld_out, int64_t ldf_out, void* stream);
int crlot_beamform(crlot_beamformer* bf, const float* d_x, int64_t ld_x, const float* d_mask, int64_t ld_mask,
                   int64_t ldf_mask, float* d_y, int64_t ld_y, int32_t n_groups, int64_t T, void* stream);
int crlot_stream_beamform_hop(crlot_stream* st_in, crlot_stream* st_out, crlot_beamformer* bf, const float* d_hop_in,
                              const float* d_mask, int64_t ld_mask, float* d_hop_out, int32_t* emitted, void* stream);

/* ---------------------------------------------------------------- dereverberation
 * Weighted prediction error (WPE; Nakatani et al. 2010, Yoshioka & Nakatani 2012; the
 * recursive form as nara_wpe's OnlineWPE): G independent groups of M microphones, the late
 * reverberation predicted from K delayed frames of all M spectra and subtracted.  The
 * input is spectra in crlot_stft's layout, the output M spectra per group in the same
 * layout, which is what crlot_beamform_accumulate / crlot_stream_beamform_hop and
 * crlot_istft_ola take.  The reference project has no dereverberation: nothing in this
 * section restates it, and no entry below cites it.
 *
 * Terms.  1 <= M <= 8 microphones, 1 <= K <= 16 taps, L = M K <= 64, delay 1 <= D <= 8.
 * Stream g M + m is microphone m of group g.  Frame t of stream s is at d_spec + s ld_spec +
 * t ldf_spec, N/2+1 float pairs; a frame before the start of the signal (t < 0) is a row of
 * zeros.  The stacked vector y~(t) of a (group, bin) has L entries, entry l = tau M + m
 * (tau = 0 .. K-1) equal to Y_m(t - D - tau).  Every entry below that walks frames takes the
 * half-open run [f0, f1) of a buffer that holds frames 0 .. f1-1: cut and carry is two
 * calls on the same buffer.
 *
 * Values.  float32, every product, sum, difference and quotient rounded on its own (no
 * FMA), division and sqrtf correctly rounded; max(a, b) is a > b ? a : b; tiny = 1e-30f; the
 * three complex products as the beamformer's section words them; |z|^2 = (re re) + (im im).
 *   1  power.  p = |Z_0|^2, then + |Z_m|^2 in m order; lambda = max(p / float(M), floor_f32);
 *      iota = 1 / lambda.  Z is the observation on the first iteration and the previous
 *      iteration's estimate afterwards.  The stored row is iota: group g, frame t, bin b at
 *      d_pow[g ld_pow + t ldf_pow + b].
 *   2  accumulate (Welch sums only), frames in order, every plane S = S + (iota T).  R_ij
 *      averages y~_i conj(y~_j): the diagonal T = (re re) + (im im); i < j: T = y~_i conj(y~_j).
 *      P_lm averages y~_l conj(Y_m(t)) by the same product.  The state block is
 *      [group][L L + 2 L M][N/2+1]: R as the beamformer stores a Hermitian matrix (the L
 *      diagonals, then Re, Im of every i < j in lexicographic order), then P as Re, Im
 *      planes, l-major (plane L L + 2 (l M + m)).  All 0 after create / reset.
 *   3  solve.  tr = R_00, then + R_ll in order; ld = max(loading_f32 (tr / float(L)), tiny);
 *      A = R + ld I; Cholesky, forward and back substitution exactly as the beamformer's
 *      step 3 words them with M replaced by L; one solve per column m of P (m ascending;
 *      the columns are independent) gives the taps G = A^-1 P, a block [group][L][M][N/2+1]
 *      float pairs, zero after create / reset (the filter then passes Y through).  No term
 *      of this step starts from a literal zero.
 *   4  filter.  acc = (0, 0); for l ascending acc = acc + conj(G_lm) y~_l(t) per component;
 *      X_m(t) = Y_m(t) - acc per component.  The imaginary parts of DC and Nyquist are stored
 *      as computed.
 *   5  RLS step for frame t.  Q (the inverse correlation matrix, Hermitian, L L planes as R)
 *      is the identity and the taps zero after create / reset.  pred_m by step 4 with the
 *      old taps: this is the output.  lambda by step 1 on Y(t).  v_i = sum over j of Q_ij y~_j,
 *      starting from j = 0's term and adding j = 1 .. in order; for i > j the conjugate of
 *      the stored entry (conj(Q_ji) y~_j), for i < j Q_ij y~_j, the diagonal term (q y.re,
 *      q y.im).  s = (y~_0.re v_0.re) + (y~_0.im v_0.im), then + the same of i = 1 .. in order;
 *      den = max((alpha_f32 lambda) + s, tiny); k_i = v_i / den per component; Q_ij = (Q_ij -
 *      k_i conj(v_j)) / alpha_f32 for i < j per component, Q_ii = (Q_ii - ((k_i.re v_i.re) +
 *      (k_i.im v_i.im))) / alpha_f32; G_lm = G_lm + k_l conj(pred_m).
 * Orders this contract fixes where the proposal left them open: the stored power row is
 * iota, not lambda; v and s start from their first term, not from zero; Q's lower triangle
 * is never stored or updated.  Output bits do not depend on the grid, the group count, a
 * group's position, the leading dimensions, where a run along the frame axis is cut, or
 * how matrix entries are spread over lanes, waves or launches.
 *
 * loading (default 1e-3) is relative to trace / L.  With 1e-3 the condition number of A
 * stays within float32's reach (3e4 on a reverberant test scene); 1e-6 does not (2e7):
 * keep the default unless the statistics are known to be well conditioned.
 *
 * crlot_wpe_create(plan, desc, groups, out) touches no device.  The descriptor is checked
 * first, with no plan needed: mics outside 1..8, taps outside 1..16, mics taps > 64, delay
 * outside 1..8, iterations outside 1..10, alpha NaN or outside (0, 1], loading NaN / Inf /
 * < 0, floor NaN / Inf / <= 0 are CRLOT_EINVAL; then a null argument, groups < 1, a size or
 * grid that does not fit.  prepare, or the first call that needs it, makes one
 * allocation: the state, Q, the taps, the v rows, the solve's workspace, and the ring and
 * the prediction rows of the per-hop entry (which forms its power inline).  _state, _inv_cov and _taps
 * return device pointers the caller may read and write; _reset synchronises the device,
 * zeroes the state, the ring, the taps and the frame counter and sets Q to the identity.
 * A single-owner object like crlot_stream; graph capture is not supported.
 *
 * crlot_wpe_power(wpe, d_z, ld_z, ldf_z, n_groups, f0, f1, d_pow, ld_pow, ldf_pow, stream):
 * step 1 (CRLOT_K_WPE_POWER).  crlot_wpe_accumulate(wpe, d_spec, ld_spec, ldf_spec, d_pow,
 * ld_pow, ldf_pow, n_groups, f0, f1, carry, d_state_out, stream): step 2 (CRLOT_K_WPE_ACC).
 * carry = 0: every group starts from zero, any n_groups, the result goes to d_state_out
 * (required), the object is untouched.  carry = 1: n_groups must equal the object's; the
 * run continues from the object's state and advances its frame counter; d_state_out may
 * be NULL (else it receives a copy).  crlot_wpe_solve(wpe, d_state, n_groups, d_taps,
 * stream): step 3 (CRLOT_K_WPE_SOLVE) in the object's workspace, so n_groups may not exceed
 * the object's; NULL for a block means the object's (then n_groups must equal the
 * object's).  crlot_wpe_filter(wpe, d_spec, ld_spec, ldf_spec, d_taps, n_groups, f0, f1,
 * d_out, ld_out, ldf_out, stream): step 4 (CRLOT_K_WPE_FILTER), frame t of stream s at d_out
 * + s ld_out + t ldf_out.  crlot_wpe_rls(wpe, d_spec, ld_spec, ldf_spec, f0, f1, d_out, ld_out,
 * ldf_out, stream): step 5 on the object's Q and taps for the object's group count, one
 * CRLOT_K_WPE_GAIN and one CRLOT_K_WPE_UPDATE launch per frame, looped on the host; the
 * frame counter advances.  n_groups of 0 or an empty run: CRLOT_OK, nothing written.
 * CRLOT_EINVAL: null buffers, f0 < 0, a leading dimension too small or (spectra) odd,
 * outputs that overlap an input, the state or the taps.
 *
 * crlot_wpe(wpe, d_x, ld_x, d_y, ld_y, n_groups, T, stream) = crlot_stft of the n_groups M
 * signals (stream s at d_x + s ld_x) -> iterations x (power of the observation, then of the
 * last estimate -> accumulate from zero -> solve -> filter) -> crlot_istft_ola of the
 * n_groups M estimates (stream s at d_y + s ld_y, F H samples).  Everything between stays in
 * the stream's sliced workspace, sliced by group; bit for bit the hand composition under
 * either frame-pairing setting.  The object is untouched.  A plan that holds a stored
 * spectral mask is CRLOT_EINVAL.
 *
 * crlot_stream_wpe_hop(st_in, st_out, wpe, d_hop_in, d_hop_out, emitted, stream): one hop of
 * the per-hop chain.  Both streams have groups M channels and are in split mode on the
 * object's plan (st_in's analysis half, st_out's synthesis half).  A hop =
 * crlot_stream_stft_hop into the object's ring of D + K rows per channel -> gain -> update
 * -> crlot_stream_istft_hop of the prediction rows: bit for bit stft_hop -> crlot_wpe_rls
 * over that one frame -> istft_hop.  A hop that completes no frame runs only the analysis
 * half, leaves d_hop_out untouched and sets *emitted = 0 (else the hop size).
 * CRLOT_EINVAL: channel counts or plans that do not match; CRLOT_ERUNTIME: frame counters
 * that differ (reset all three), a stream in whole-hop mode.  crlot_wpe_last_launch lists
 * the last call's kernels and grids (crlot_wpe: the last iteration's four; crlot_wpe_rls:
 * the last frame's two). */
typedef struct crlot_wpe_desc {
    int32_t mics;        /* M, 1..8 */
    int32_t taps;        /* K, 1..16, M K <= 64 */
    int32_t delay;       /* D, 1..8 */
    int32_t iterations;  /* 1..10: crlot_wpe's passes (default 3) */
    double alpha;        /* (0, 1]: the RLS forgetting factor (default 0.9999) */
    double loading;      /* >= 0, finite: diagonal loading relative to trace / L (default 1e-3) */
    double floor;        /* > 0, finite: the power floor (default 1e-10) */
} crlot_wpe_desc;
typedef struct crlot_dereverberator crlot_dereverberator;
typedef struct crlot_wpe_launch {
    int32_t n_kernels;  /* 0: no launch yet */
    int32_t kernel[4];  /* CRLOT_K_* in launch order */
    int32_t reserved;
    int64_t grid[4];    /* workgroups of each */
} crlot_wpe_launch;
int crlot_wpe_desc_default(crlot_wpe_desc* d);
int crlot_wpe_create(crlot_plan* plan, const crlot_wpe_desc* desc, int32_t groups, crlot_dereverberator** out);
void crlot_wpe_destroy(crlot_dereverberator* wpe);
int crlot_wpe_prepare(crlot_dereverberator* wpe);
int crlot_wpe_reset(crlot_dereverberator* wpe);
int crlot_wpe_info(const crlot_dereverberator* wpe, int32_t* groups, int32_t* mics, int32_t* taps, int32_t* delay,
                   int32_t* iterations, int32_t* bins, int64_t* frames, float* alpha, float* loading, float* floor);
int crlot_wpe_state(crlot_dereverberator* wpe, float** d_state /* [groups][L L + 2 L M][N/2+1] */);
int crlot_wpe_inv_cov(crlot_dereverberator* wpe, float** d_q /* [groups][L L][N/2+1] */);
int crlot_wpe_taps(crlot_dereverberator* wpe, float** d_taps /* [groups][L][M][N/2+1] float pairs */);
int crlot_wpe_last_launch(const crlot_dereverberator* wpe, crlot_wpe_launch* out);
int crlot_wpe_power(crlot_dereverberator* wpe, const float* d_z, int64_t ld_z, int64_t ldf_z, int32_t n_groups, int64_t f0,
                    int64_t f1, float* d_pow, int64_t ld_pow, int64_t ldf_pow, void* stream);
int crlot_wpe_accumulate(crlot_dereverberator* wpe, const float* d_spec, int64_t ld_spec, int64_t ldf_spec, const float* d_pow,
                         int64_t ld_pow, int64_t ldf_pow, int32_t n_groups, int64_t f0, int64_t f1, int32_t carry,
                         float* d_state_out /* carry = 1: may be NULL */, void* stream);
int crlot_wpe_solve(crlot_dereverberator* wpe, const float* d_state /* NULL: the object's */, int32_t n_groups,
                    float* d_taps /* NULL: the object's */, void* stream);
int crlot_wpe_filter(crlot_dereverberator* wpe, const float* d_spec, int64_t ld_spec, int64_t ldf_spec,
                     const float* d_taps /* NULL: the object's */, int32_t n_groups, int64_t f0, int64_t f1,
                     float* d_out, int64_t ld_out, int64_t ldf_out, void* stream);
int crlot_wpe_rls(crlot_dereverberator* wpe, const float* d_spec, int64_t ld_spec, int64_t ldf_spec, int64_t f0, int64_t f1,
                  float* d_out, int64_t ld_out, int64_t ldf_out, void* stream);
int crlot_wpe(crlot_dereverberator* wpe, const float* d_x, int64_t ld_x, float* d_y, int64_t ld_y, int32_t n_groups, int64_t T,
              void* stream);
int crlot_stream_wpe_hop(crlot_stream* st_in, crlot_stream* st_out, crlot_dereverberator* wpe, const float* d_hop_in,
                         float* d_hop_out, int32_t* emitted, void* stream);

/* host helpers (no device) */
#define CRLOT_MEL_HTK 0
#define CRLOT_MEL_SLANEY 1
/* Triangular mel filterbank, computed in double and rounded once to float: n_mels + 2 points
 * equally spaced on the mel scale between fmin and fmax (fmax <= 0: sample_rate / 2); HTK
 * mel = 2595 log10(1 + f/700); Slaney linear f / (200/3) below 1000 Hz, logarithmic above with
 * step ln(6.4)/27.  Bin b has frequency b sample_rate / nfft and weight
 * max(0, min((f - f_lo)/(f_c - f_lo), (f_hi - f)/(f_hi - f_c))); slaney_norm multiplies row j by
 * 2/(f_hi - f_lo).  CRLOT_EINVAL: n_mels < 1, nfft odd or < 2, not 0 <= fmin < fmax <= sample_rate/2. */
int crlot_mel_filterbank(int32_t n_mels, int32_t nfft, double sample_rate, double fmin, double fmax,
                         int32_t scale, int32_t slaney_norm, float* out /* [n_mels][nfft/2+1] */);
/* lo[j], hi[j]: row j's span (first to one past the last non-zero weight; all zero: 0, 0) */
int crlot_filterbank_spans(const float* weights, int32_t n_bands, int32_t bins, int32_t* lo, int32_t* hi);

/* Batched IFftPlan::forward / inverse with the adapter's semantics
 * (kissfft_adapter.cc:83-168): forward sanitizes its input, inverse scales by
 * 1/N and sanitizes its output.  Element i of batch b lives at
 * [b*ld + i*inc] (float for real data, float pairs for spectra). */
int crlot_rfft_batched(crlot_plan* plan, const float* d_in, float* d_out_complex, int32_t batch,
                       int64_t ld_in, int64_t inc_in, int64_t ld_out, int64_t inc_out,
                       void* stream);
int crlot_irfft_batched(crlot_plan* plan, const float* d_in_complex, float* d_out, int32_t batch,
                        int64_t ld_in, int64_t inc_in, int64_t ld_out, int64_t inc_out,
                        void* stream);

/* ---------------------------------------------------------------- FFT plans
 * dsp::fft::MakeFftPlan / IFftPlan (fft_api.h:16-51; kissfft_adapter.cc:11-269)
 * as a device object of its own, both domains.  Semantics per entry point:
 *   forward          real, sanitized input -> nfft/2+1 bins   (adapter :83-122)
 *   inverse          nfft/2+1 bins -> real, *1/nfft, sanitize  (adapter :124-168)
 *   forward_complex  complex -> complex, unnormalised, no sanitize (adapter :171-201)
 *   inverse_complex  complex -> complex, *1/nfft, sanitize     (adapter :204-246)
 * Calling the other domain's entry is CRLOT_ERUNTIME with the reference's
 * message.  Element i of batch b is at [b*ld + i*inc] (ld in floats, inc in
 * elements: floats for real data, float pairs for complex).  Sizes: real nfft
 * even in 2..16384, complex nfft 1..8192 (any factorisation, as kiss_fft);
 * larger sizes are CRLOT_EUNSUPPORTED.  No batch ceiling on the device path;
 * MakeFftPlan's 1..16 rule is applied by the C++ layer (crlot_dsp.hpp). */
#define CRLOT_FFT_REAL 0
#define CRLOT_FFT_COMPLEX 1
typedef struct crlot_fft_plan crlot_fft_plan;
typedef struct crlot_fft_desc {
    int32_t domain; /* CRLOT_FFT_REAL / CRLOT_FFT_COMPLEX (FftPlanDesc::domain) */
    int32_t nfft;   /* FftPlanDesc::nfft */
    int32_t device; /* HIP device ordinal, -1 = current */
} crlot_fft_desc;
int crlot_fft_plan_create(const crlot_fft_desc* desc, crlot_fft_plan** out);
void crlot_fft_plan_destroy(crlot_fft_plan* plan);
int crlot_fft_plan_info(const crlot_fft_plan* plan, int32_t* domain, int32_t* nfft);
int crlot_fft_forward(crlot_fft_plan* plan, const float* d_in, float* d_out_complex, int32_t batch,
                      int64_t ld_in, int64_t inc_in, int64_t ld_out, int64_t inc_out, void* stream);
int crlot_fft_inverse(crlot_fft_plan* plan, const float* d_in_complex, float* d_out, int32_t batch,
                      int64_t ld_in, int64_t inc_in, int64_t ld_out, int64_t inc_out, void* stream);
int crlot_fft_forward_complex(crlot_fft_plan* plan, const float* d_in_complex, float* d_out_complex,
                              int32_t batch, int64_t ld_in, int64_t inc_in, int64_t ld_out,
                              int64_t inc_out, void* stream);
int crlot_fft_inverse_complex(crlot_fft_plan* plan, const float* d_in_complex, float* d_out_complex,
                              int32_t batch, int64_t ld_in, int64_t inc_in, int64_t ld_out,
                              int64_t inc_out, void* stream);

/* Host-pointer forms of the four transforms: the reference's own calling
 * convention (IFftPlan::forward(const float*, complex<float>*, batch) etc.),
 * synchronous, data in host memory, same semantics and layout parameters as
 * the device forms.  Power-of-two plans (real nfft 256..4096, complex
 * 128..2048) run on a resident server kernel owned by the plan (call_rt.hip):
 * no kernel launch and no copy-engine transfer per call, the input written into
 * fine-grained device memory through the BAR, the result written by the kernel
 * into pinned host memory.  After a real forward of batch <= 4 the server also
 * runs the inverse of the spectrum it returned; an inverse called next with
 * exactly those bits (memcmp) is served from that result (bit-identical to
 * running it).  The server exits after 20 ms without a call.  Other sizes stage
 * through device buffers and a launch. */
int crlot_fft_forward_host(crlot_fft_plan* plan, const float* in, float* out_complex, int32_t batch,
                           int64_t ld_in, int64_t inc_in, int64_t ld_out, int64_t inc_out);
int crlot_fft_inverse_host(crlot_fft_plan* plan, const float* in_complex, float* out, int32_t batch,
                           int64_t ld_in, int64_t inc_in, int64_t ld_out, int64_t inc_out);
int crlot_fft_forward_complex_host(crlot_fft_plan* plan, const float* in_complex, float* out_complex,
                                   int32_t batch, int64_t ld_in, int64_t inc_in, int64_t ld_out,
                                   int64_t inc_out);
int crlot_fft_inverse_complex_host(crlot_fft_plan* plan, const float* in_complex, float* out_complex,
                                   int32_t batch, int64_t ld_in, int64_t inc_in, int64_t ld_out,
                                   int64_t inc_out);

/* ---------------------------------------------------------------- streaming
 * Low-latency per-hop path (BASELINE config 4): `channels` independent
 * channels, Framer in DROP mode fed H samples per channel per call
 * (Framer::push of one hop then pop, OLAAccumulator push_frame_AoS + produce(H);
 * framer.cc:37-117, OLAAccumulator.cc:124-221).  Each call consumes d_hop_in
 * and, once N samples per channel have arrived, writes the next H output
 * samples per channel into d_hop_out; *emitted (host) gets 0 or H.  Layout:
 * channel-major [channels][H] by default, or interleaved [H][channels] (the
 * reference's interleaved PCM) after crlot_stream_set_layout(st, 1).  Device
 * state (the recent input samples, the OLA blocks) persists across calls.  Any
 * N / H the plan accepts: H % 128 == 0, N % H == 0, N <= 2048 run the
 * register-resident per-hop kernel, other shapes the mixed-radix one. */
int crlot_stream_create(crlot_plan* plan, int32_t channels, crlot_stream** out);
void crlot_stream_destroy(crlot_stream* st);
int crlot_stream_reset(crlot_stream* st);
int crlot_stream_set_layout(crlot_stream* st, int32_t interleaved);
int crlot_stream_push_hop(crlot_stream* st, const float* d_hop_in, float* d_hop_out,
                          int32_t* emitted, void* stream);

/* The per-hop path with a time-varying spectral step (a suppressor, a Wiener
 * gain, a mask model that looks at frame k and edits frame k before it is
 * synthesised): the hop cut at its spectrum, and the hop with a mask row.
 * Numerics are the batched entries', operation for operation (crlot_stft,
 * crlot_istft_ola, crlot_roundtrip with a mask): sanitize(x * wa), forward,
 * kiss_fftr split; the step (X * gain) * mask in float32 on re and im each;
 * kiss_fftri merge, * 1/N, sanitize, fma(fma(o, ws, 0), g, acc), IEEE / den.
 * Spectra are channel-major whatever the PCM layout: channel c's N/2+1 float
 * pairs at d_spec[c*ld_spec + 2*b], ld_spec even and >= N + 2, d_spec 8-byte
 * aligned; DC / Nyquist imaginary parts are 0 on the way out and ignored on the
 * way in.  A mask row holds N/2+1 real floats, channel c's at d_mask[c*ld_mask];
 * ld_mask = 0 shares one row across the channels, otherwise ld_mask >= N/2+1;
 * d_mask = NULL: no mask.  Violations are CRLOT_EINVAL.
 *   stft_hop         the analysis half of push_hop: consume H samples per channel
 *                    (layout as push_hop); when the hop completes DROP frame f,
 *                    write its spectrum -- frame * analysis window ->
 *                    IFftPlan::forward, BEFORE the gain: crlot_stft's row f.
 *                    *emitted = 1 if a spectrum was written, else 0 (d_spec untouched).
 *   istft_hop        the synthesis half: one spectrum per channel -> (X * gain) *
 *                    mask row (either may be absent) -> IFftPlan::inverse ->
 *                    push_frame_AoS(k*H) -> produce(H): always writes block k (H
 *                    samples per channel, hop layout), k = istft_hop calls so far.
 *   push_hop_masked  push_hop with a mask row for the frame this hop completes
 *                    (read only on a hop that emits): one launch, no spectra in
 *                    HBM; equal bit for bit to istft_hop(stft_hop(hop)), and to
 *                    push_hop with a row of ones or d_mask = NULL.
 * An object's first call after create / reset fixes its mode: whole (push_hop and
 * push_hop_masked, freely mixed) or split (stft_hop and istft_hop, whose two
 * halves keep independent counters -- hops analysed, frames synthesised -- and
 * share nothing but the plan and the object).  A call of the other mode is
 * CRLOT_ERUNTIME until crlot_stream_reset, which clears both counters and the
 * mode.  The hop / frame index is a by-value kernel argument, so a captured
 * graph of one hop replays that hop: capture is not supported on this path. */
int crlot_stream_stft_hop(crlot_stream* st, const float* d_hop_in, float* d_spec, int64_t ld_spec,
                          int32_t* emitted, void* stream);
int crlot_stream_istft_hop(crlot_stream* st, const float* d_spec, int64_t ld_spec, const float* d_mask,
                           int64_t ld_mask, float* d_hop_out, void* stream);
int crlot_stream_push_hop_masked(crlot_stream* st, const float* d_hop_in, const float* d_mask, int64_t ld_mask,
                                 float* d_hop_out, int32_t* emitted, void* stream);

/* Per-hop spectrogram features: stft_hop's analysis half with the features of a
 * crlot_features object (created on the stream's plan) computed where the
 * spectrum row would be stored -- what a mask model, a VAD or a streaming
 * recogniser is fed -- in the same single launch.  Consumes H samples per
 * channel (layout as push_hop); when the hop completes DROP frame k, channel c's
 * n_out floats go to d_feat[c*ld_feat + j], channel-major whatever the PCM
 * layout, ld_feat >= n_out, and *emitted = 1; otherwise *emitted = 0 and d_feat
 * and d_spec are untouched.  d_spec != NULL: the launch also writes the spectrum
 * row exactly as crlot_stream_stft_hop does (same layout rules and checks), so
 * istft_hop(spec, mask(features)) can follow with no second analysis; d_spec =
 * NULL: no spectrum reaches HBM and ld_spec is ignored.  A split-mode call: it
 * advances stft_hop's hop counter and mixes freely with stft_hop; on a whole-mode
 * object it is CRLOT_ERUNTIME until crlot_stream_reset.  CRLOT_EINVAL: a null st,
 * f, d_hop_in or d_feat; f created on another plan than st's; ld_feat < n_out; a
 * non-NULL d_spec that fails stft_hop's checks.  The features object is read
 * stream-ordered and must outlive every hop enqueued with it.  Graph capture is
 * not supported, as on the rest of this path.
 * Value contract: X is bit for bit the row crlot_stream_stft_hop writes for that
 * hop -- the per-frame transform, before the plan gain, no sanitize after the
 * forward; the plan's frame-pairing setting plays no part (the hop path has no
 * pairs).  From X onward the contract is crlot_spectrogram's, line for line:
 * p = fl(fl(re re) + fl(im im)) with no FMA; the correctly rounded sqrtf for
 * MAGNITUDE; the span / 8-part / tree summation order for bands; logf / log10f /
 * 10 log10f of fmaxf(v, floor) of exactly the LIN value.  Output bits do not
 * depend on the channel count, the PCM layout, ld_feat, whether d_spec is given,
 * or where the kernel reads the filterbank from. */
int crlot_stream_features_hop(crlot_stream* st, const crlot_features* f, const float* d_hop_in, float* d_feat,
                              int64_t ld_feat, float* d_spec, int64_t ld_spec, int32_t* emitted, void* stream);

/* ---------------------------------------------------------------- resident streaming
 * The same per-hop contract as crlot_stream_* (DROP Framer fed H samples per
 * channel per hop, push_frame_AoS + produce(H); framer.cc:37-117,
 * OLAAccumulator.cc:124-221; bit-identical outputs) for real-time callers whose
 * hops live in HOST memory (BASELINE config 4, the ring-buffer low-latency path).
 * One kernel stays resident on the device with the tables in LDS and each
 * channel's state in registers; hops travel through pinned host rings of
 * `depth` slots (0 -> 4) with a doorbell, so a hop costs no kernel launch and no
 * copy-engine transfer.  The kernel exits after 20 ms without a hop (or on
 * reset / destroy / a plan table update) and is relaunched by the next hop; a
 * hipDeviceSynchronize elsewhere in the process therefore waits at most that
 * idle time.  N in 256..2048, H % 128 == 0, N % H == 0, channels 1..1024.
 * Every other shape the plan streams (960/480, 882/441 ...) gets the same
 * contract in launch mode: per hop an H2D copy of the slot, the per-launch hop
 * kernel (crlot_stream_push_hop's, bit-identical), a D2H copy and an event; no
 * resident kernel (info reports last_device_ns 0, running 0).
 *   push_hop      copy h_in into the next slot, submit, wait, copy the H output
 *                 samples per channel into h_out (*emitted = 0 or H); h_in /
 *                 h_out are [H][C] interleaved PCM if `interleaved`, else [C][H]
 *   input_slot    zero-copy form: the host slot for the next hop (C*H floats,
 *                 always channel-major [C][H]), then submit -> hop index,
 *                 wait -> pointer to that hop's [C][H] output slot (valid until hop
 *                 index + depth is submitted); up to `depth` hops in flight
 *   info          hops submitted, the device time of the last hop (ns, from the
 *                 kernel's own clock: doorbell seen -> output published), running */
typedef struct crlot_stream_rt crlot_stream_rt;
int crlot_stream_rt_create(crlot_plan* plan, int32_t channels, int32_t interleaved, int32_t depth,
                           crlot_stream_rt** out);
void crlot_stream_rt_destroy(crlot_stream_rt* st);
int crlot_stream_rt_reset(crlot_stream_rt* st);
int crlot_stream_rt_push_hop(crlot_stream_rt* st, const float* h_hop_in, float* h_hop_out,
                             int32_t* emitted);
float* crlot_stream_rt_input_slot(crlot_stream_rt* st);
int crlot_stream_rt_submit(crlot_stream_rt* st, int64_t* hop_index);
int crlot_stream_rt_wait(crlot_stream_rt* st, int64_t hop_index, const float** h_hop_out,
                         int32_t* emitted);
int crlot_stream_rt_info(const crlot_stream_rt* st, int64_t* hops, double* last_device_ns,
                         int32_t* running);
/* diagnostic: workgroup 0's phase times of the last hop (ns after the doorbell
 * was seen: hop read issued, hop staged, transform done, output barrier, output
 * issued, release fence, publish barrier); zeros unless the library was built
 * with -DCRLOT_RT_PHASES */
int crlot_stream_rt_phases(const crlot_stream_rt* st, double* ns8);
/* idle exit after `idle_seconds` without a hop; a wait fails (CRLOT_EHIP) after
 * `hop_timeout_seconds` (defaults 0.02 and 2) */
int crlot_stream_rt_set_idle_timeout(crlot_stream_rt* st, double idle_seconds,
                                     double hop_timeout_seconds);

/* ---------------------------------------------------------------- Framer (host)
 * dsp::Framer (framer.h:26-127, framer.cc:15-181): interleaved PCM of
 * `channels` channels in, frames of frame_size*channels interleaved samples out
 * every hop_size samples per channel; ZERO_PAD pads the last partial frame with
 * zeros, DROP never emits one.  A host object (bookkeeping and copies); the
 * batched crlot_roundtrip frames on the device instead.
 * push / pop return 1 (true) or 0 (false) as the reference's bool, negative on
 * a bad handle; set_params fails with CRLOT_EINVAL and the reference's message
 * (std::invalid_argument) on a zero size. */
typedef struct crlot_framer crlot_framer;
int crlot_framer_create(crlot_framer** out);
void crlot_framer_destroy(crlot_framer* f);
int crlot_framer_set_params(crlot_framer* f, int64_t frame_size, int64_t hop_size, int64_t channels,
                            int32_t boundary_mode);
int crlot_framer_push(crlot_framer* f, const float* interleaved, int64_t frames);
int crlot_framer_pop(crlot_framer* f, float* out_frame);
int64_t crlot_framer_available(const crlot_framer* f);
int crlot_framer_reset(crlot_framer* f);
int crlot_framer_info(const crlot_framer* f, int64_t* frame_size, int64_t* hop_size,
                      int64_t* channels, int32_t* boundary_mode, int64_t* buffer_size);

/* ---------------------------------------------------------------- OLAAccumulator
 * dsp::OLAAccumulator (OLAAccumulator.h:15-217, OLAAccumulator.cc:13-295) with
 * its state on the device: per-channel rings [channels][ring_len] and the COLA
 * divisors in HBM, every add / produce a kernel; the host keeps the reference's
 * counters (produced_samples, read_pos, flush, reset) so any call sequence
 * behaves as the reference's.  Per-sample arithmetic is the reference's scalar
 * kernels (kernels.cc:18-36): fma(fma(x, w, 0), gain, acc) or fma(x, gain, acc);
 * out = acc / (norm > eps ? norm : eps), acc = 0.
 * Two call forms: host pointers (the reference's signatures) run on a resident
 * server kernel owned by the object (call_rt.hip): an add is posted without
 * waiting, produce() returns when the samples are in the caller's buffers; after
 * each add the server also computes the produce(n) block the object predicts
 * (n of the previous produce, H before the first), without clearing, and a
 * produce asking for exactly that block is served from it (the ring is cleared
 * by a request behind it).  _device forms run on caller-owned HBM with a stream
 * (NULL = the object's stream); calls on different streams, and switches between
 * the two forms, are ordered by the object.  Null pointers fail with CRLOT_EINVAL and the reference's
 * messages.  Not thread-safe (as the reference). */
typedef struct crlot_ola crlot_ola;
typedef struct crlot_ola_config { /* dsp::OLAConfig (OLAAccumulator.h:15-29) */
    int32_t sample_rate;
    int64_t frame_size;
    int64_t hop_size;
    int64_t channels;
    float eps;                   /* reference default 1e-8f */
    int32_t apply_window_inside;
    int32_t shadow_ring;         /* accepted; value-neutral (ola_accumulator_test.cc:1079-1120) */
    int32_t device;              /* HIP device ordinal, -1 = current */
} crlot_ola_config;
int crlot_ola_create(const crlot_ola_config* cfg, crlot_ola** out);
void crlot_ola_destroy(crlot_ola* o);
int crlot_ola_set_window(crlot_ola* o, const float* window, int32_t wlen);
/* ch_frames[c] (host), c < channels */
int crlot_ola_add_frame_soa(crlot_ola* o, const float* const* ch_frames, const float* window,
                            int64_t start_sample, int64_t start_off, int64_t size, float gain);
/* interleaved [frame_size][channels] (host) */
int crlot_ola_push_frame_aos(crlot_ola* o, const float* interleaved, const float* window,
                             int64_t start_sample, int64_t start_off, int64_t size, float gain);
/* ch_out[c] (host) receives up to n samples; *n_out = samples provided */
int crlot_ola_produce(crlot_ola* o, float* const* ch_out, int64_t n, int64_t* n_out);
/* device forms: channel c of a frame at d_frames + c*ld_frames; window (when the
 * object does not apply its own) a device array of frame_size floats */
int crlot_ola_add_frame_soa_device(crlot_ola* o, const float* d_frames, int64_t ld_frames,
                                   const float* d_window, int64_t start_sample, int64_t start_off,
                                   int64_t size, float gain, void* stream);
int crlot_ola_push_frame_aos_device(crlot_ola* o, const float* d_interleaved, const float* d_window,
                                    int64_t start_sample, int64_t start_off, int64_t size, float gain,
                                    void* stream);
/* channel c written to d_out + c*ld_out (n floats per channel must be valid) */
int crlot_ola_produce_device(crlot_ola* o, float* d_out, int64_t ld_out, int64_t n, int64_t* n_out,
                             void* stream);
int crlot_ola_flush(crlot_ola* o);
int crlot_ola_reset(crlot_ola* o);
int crlot_ola_info(const crlot_ola* o, int64_t* produced_samples, int64_t* read_pos,
                   int64_t* ring_size, int32_t* has_window);
/* channel-0 peak of every sample produced so far (waits for device produces) */
int crlot_ola_meter_peak(crlot_ola* o, float* peak);
/* the object's COLA norm table (ring_size floats, before the eps guard) */
int crlot_ola_norm_table(const crlot_ola* o, float* out);
/* wait for everything issued on the object */
int crlot_ola_synchronize(crlot_ola* o);

/* ---------------------------------------------------------------- OLA kernels
 * dsp::axpy / axpy_windowed / normalize_and_clear (ola/kernels.h:28-53; scalar
 * forms kernels.cc:18-36, which the Highway forms match) as batched device
 * entries: `batch` rows of n elements, row b of dst / src / out / acc at
 * + b*ld; the window (axpy_windowed) and the norm row (normalize_and_clear) are
 * one row of n shared by every row.  Per element, bit-exact with the reference:
 *   axpy               dst = fma(src, g, dst)
 *   axpy_windowed      dst = fma(fma(src, win, 0), g, dst)
 *   normalize_and_clear out = acc / (norm > eps ? norm : eps), acc = 0
 * batch <= 65535.
 * crlot_call_*: the reference's host-pointer signatures (n elements in host
 * memory, synchronous), run on a per-device resident server kernel
 * (call_rt.hip); normalize_and_clear also zeroes acc, as the reference. */
int crlot_axpy(float* d_dst, const float* d_src, float g, int64_t n, int64_t batch, int64_t ld_dst,
               int64_t ld_src, void* stream);
int crlot_axpy_windowed(float* d_dst, const float* d_src, const float* d_win, float g, int64_t n,
                        int64_t batch, int64_t ld_dst, int64_t ld_src, void* stream);
int crlot_normalize_and_clear(float* d_out, float* d_acc, const float* d_norm, float eps, int64_t n,
                              int64_t batch, int64_t ld_out, int64_t ld_acc, void* stream);
int crlot_call_axpy(float* dst, const float* src, float g, int64_t n);
int crlot_call_axpy_windowed(float* dst, const float* src, const float* win, float g, int64_t n);
int crlot_call_normalize_and_clear(float* out, float* acc, const float* norm, float eps, int64_t n);

/* ---------------------------------------------------------------- FrameQueue
 * dsp::FrameQueue (FrameQueue.h:35-59, FrameQueue.cc:9-115, Indexing.h:18-70):
 * all frames of a whole signal, padded by N/2 on both sides when `center`
 * (CRLOT_PAD_CONSTANT zeros / REFLECT reflect-101 / EDGE), frame k = padded
 * samples [k*H, k*H + N), count floor((len + pad - max(N - H, 0)) / H) on the
 * padded length.  The object builds the frames on the device at construction
 * (device_frames: [num_frames][N] in HBM) and keeps the reference's AoS host
 * copy for frame / copy_frame / all_frames.  Errors: CRLOT_EINVAL with the
 * reference's std::invalid_argument messages, CRLOT_ERANGE for a frame index
 * out of range (std::out_of_range; crlot_framequeue_frame returns NULL).
 * crlot_framequeue_frames is the batched device form: n_streams streams of T
 * samples at d_x + s*ld_x -> d_frames [s][count][frame_size]. */
typedef struct crlot_framequeue crlot_framequeue;
int64_t crlot_framequeue_count(int64_t T, int64_t frame_size, int64_t hop_size, int32_t center);
int crlot_framequeue_frames(const float* d_x, int32_t n_streams, int64_t T, int64_t ld_x, int64_t frame_size,
                            int64_t hop_size, int32_t center, int32_t pad_mode, float* d_frames, void* stream);
int crlot_framequeue_create(const float* in, int64_t len, int64_t frame_size, int64_t hop_size, int32_t center,
                            int32_t pad_mode, int32_t device, crlot_framequeue** out);
void crlot_framequeue_destroy(crlot_framequeue* q);
int crlot_framequeue_info(const crlot_framequeue* q, int64_t* num_frames, int64_t* frame_size,
                          int64_t* hop_size);
const float* crlot_framequeue_frame(const crlot_framequeue* q, int64_t frame_idx);
int crlot_framequeue_copy_frame(const crlot_framequeue* q, int64_t frame_idx, float* out);
const float* crlot_framequeue_all_frames(const crlot_framequeue* q);
const float* crlot_framequeue_device_frames(const crlot_framequeue* q);

/* ---------------------------------------------------------------- WAV I/O
 * io/wav.{h,cc} (WavReader / WavWriter over dr_wav): RIFF WAVE, 1 or 2
 * channels, 16/24/32-bit PCM or 32-bit IEEE float (wav.cc:26-55 guards; a
 * rejected file is CRLOT_ERUNTIME, the reference's `false`).  Samples are
 * interleaved float frames with dr_wav's conversions: s16 * 2^-15,
 * s24 * 2^-23, s32 / 2^31 on read; drwav_f32_to_s16 / the reference's 24-bit
 * packer (wav.cc:233-246) / 2^31 * x (clamped) on write.  Host memory only. */
typedef struct crlot_wav_reader crlot_wav_reader;
typedef struct crlot_wav_writer crlot_wav_writer;
int crlot_wav_reader_open(const char* path, crlot_wav_reader** out);
void crlot_wav_reader_close(crlot_wav_reader* r);
int crlot_wav_reader_info(const crlot_wav_reader* r, uint32_t* channels, uint32_t* sample_rate,
                          uint64_t* total_frames, uint32_t* bits_per_sample, int32_t* is_float);
/* reads up to `frames` frames from the current position; *frames_read < frames at the end */
int crlot_wav_reader_read(crlot_wav_reader* r, float* out, uint64_t frames, uint64_t* frames_read);
int crlot_wav_writer_open(const char* path, uint32_t channels, uint32_t sample_rate,
                          uint32_t bits_per_sample, int32_t float_format, crlot_wav_writer** out);
int crlot_wav_writer_write(crlot_wav_writer* w, const float* in, uint64_t frames, uint64_t* written);
/* patches the RIFF/data sizes and closes the file */
int crlot_wav_writer_close(crlot_wav_writer* w);

/* ---------------------------------------------------------------- host tables
 * The reference's table builders, restated in the product's host code
 * (bit-exact with WindowLUT.cc / norm_builder.cc / OLAAccumulator.cc). */
int crlot_window_table(int32_t type, int64_t n, int32_t periodic, int32_t norm, float* out);
int64_t crlot_ring_len(int64_t frame_size, int64_t hop);
int crlot_norm_table(const float* window, int64_t frame_size, int64_t hop, int64_t ring_len,
                     int32_t apply_window_inside, float eps, float* out);
/* dsp::ola::build_norm_linear (norm_builder.cc:8-52): the raw linear sum of the
 * window over every frame start that reaches the ring (no eps, no H == N case) */
int crlot_build_norm_linear(float* norm, const float* window, int64_t ring_len, int64_t frame_size, int64_t hop);
/* The device the calling thread's HIP context uses, as an ISA name ("gfx950");
 * the target of the dsp::get_current_target() drop-in */
const char* crlot_device_target(void);

#ifdef __cplusplus
}
#endif
#endif /* CRLOT_DSP_H_ */
