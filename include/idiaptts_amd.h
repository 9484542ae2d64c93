/*
 * idiaptts_amd.h -- C ABI of the MI355X-native IdiapTTS hot path (libidiaptts_amd.so).
 *
 * The reference (idiap/IdiapTTS v0.2) has no FFI of its own: the boundary is the Python call
 * surface that today delegates to pyworld / pysptk / bandmat / torch.  Every entry point below
 * cites the reference call site it replaces (paths relative to /root/reference/idiaptts).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / HIP types in signatures.
 *   - `d_*` parameters are DEVICE pointers (HBM), `h_*` are host pointers.  Buffers are
 *     caller-owned and C-contiguous unless a leading dimension is passed; the library never
 *     keeps a pointer after the call returns.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  GPU entry points are
 *     asynchronous with respect to the host unless stated otherwise.
 *   - return value: 0 = ok, negative = error (ITTS_E_*); itts_last_error() gives a message.
 *   - no hidden global state besides read-only tables cached per device (and the MLPG form override and
 *     last-form record, itts_mlpg_set_override / itts_mlpg_last_form, and the adjoint's own pair,
 *     itts_mlpg_adjoint_set_override / itts_mlpg_adjoint_last_form); HIP is not
 *     initialised before the first GPU entry point is called (fork-safe for DataLoader workers,
 *     src/neural_networks/pytorch/ModularModelHandlerPyTorch.py:528-548).
 */
#ifndef IDIAPTTS_AMD_H
#define IDIAPTTS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITTS_OK 0
#define ITTS_E_INVALID (-1)  /* bad argument (shape / size / null pointer)            */
#define ITTS_E_HIP (-2)      /* HIP runtime error, see itts_last_error()               */
#define ITTS_E_UNSUPPORTED (-3)

/* ---- library ------------------------------------------------------------------------- */
int itts_abi_version(void);
const char* itts_last_error(void);
/* number of visible HIP devices (initialises HIP). */
int itts_device_count(void);
/* Bytes of scratch the library holds on the current device (reserved), of which handed out (used),
 * and the amount it may keep between calls (ITTS_POOL_KEEP_GB); any pointer may be NULL. */
int itts_scratch_pool_stats(int64_t* reserved, int64_t* used, int64_t* keep_threshold);

/* The GPU entry points take their scratch from blocks the library keeps per device (stream-ordered:
 * a block handed back on one stream is reused on another only behind an event), up to
 * ITTS_POOL_KEEP_GB (environment, default 64) between calls.  This synchronises the device and hands
 * every idle block back, e.g. between a feature-extraction job and training in one process. */
int itts_release_scratch(void);

/* Deferred reductions (this host thread): while on, itts_linear_fwd_mse / itts_masked_mse /
 * itts_linear_bwd / itts_linear_bwd_weight leave their partial results (loss partial sums, split-K
 * slabs of the weight and bias gradients) in the workspace they were given and queue the reduction
 * they owe; itts_reduce_deferred then runs every queued reduction in ONE launch (bit-identical
 * results) and switches deferral off.  The caller keeps each call's workspace alive and separate
 * until then.  A training step of the dense stack owes five such reductions, each a launch of its own
 * otherwise (FFWrapper.py:63-73 backward + NamedLoss.py:113-117; torch launches one kernel per
 * gradient as well). */
int itts_defer_reductions(int on);
int itts_reduce_deferred(void* stream);

/* ---- gradient exchange of data-parallel training (csrc/collective.cpp) --------------------------
 * Replaces torch.nn.DataParallel's scatter / gather / gradient reduction
 * (src/neural_networks/pytorch/ModularModelHandlerPyTorch.py:732-735, :757-763) by one process per GPU
 * and an in-place all-reduce of a flat device buffer (the gradient arena, or the additive
 * normalisation sums of gen_data) over RCCL / xGMI on the caller's stream.  RCCL is resolved at run
 * time from the copy the process already holds (PyTorch's), else the system's; ITTS_E_UNSUPPORTED when
 * there is none.  A communicator is either the caller's own ncclComm_t or one made here:
 *   itts_comm_unique_id   rank 0 fills 128 bytes, sends them to the others by any means
 *   itts_comm_init_rank   collective over the n_ranks processes (device = the current HIP device)
 *   itts_allreduce_flat   d_buf[0..n) <- reduction over the ranks, in place, asynchronous on `stream`
 *   itts_comm_destroy
 *   itts_comm_version     the library's ncclGetVersion code (e.g. 22707), 0 when no usable RCCL was found: the
 *                         binding passes enum values of the 2.10+ ABI and refuses any other version */
#define ITTS_F32 0
#define ITTS_F64 1
#define ITTS_REDUCE_SUM 0
#define ITTS_REDUCE_MAX 1
#define ITTS_REDUCE_AVG 2
int itts_comm_version(void);
int itts_comm_unique_id(void* h_id128);
int itts_comm_init_rank(const void* h_id128, int n_ranks, int rank, void** comm_out);
int itts_comm_destroy(void* comm);
int itts_allreduce_flat(void* d_buf, int64_t n, int dtype, int op, void* comm, void* stream);

/* ---- integer / scalar helpers (host, no GPU) ------------------------------------------- */
/* pyworld.get_cheaptrick_fft_size(fs, f0_floor=71)  -- src/data_preparation/audio/AudioProcessing.py:60 */
int itts_cheaptrick_fft_size(int fs, double f0_floor);
/* pyworld.get_num_aperiodicities(fs)                -- AudioProcessing.py:71 */
int itts_num_aperiodicities(int fs);
/* pysptk.util.mcepalpha(fs)                         -- AudioProcessing.py:40 */
double itts_mcep_alpha(int fs);
/* number of analysis frames pyworld.wav2world yields: int(1000*n/fs/frame_period)+1 */
int64_t itts_world_num_frames(int64_t n_samples, int fs, double frame_period_ms);
/* samples pyworld.synthesize yields: int(T*frame_period*fs/1000) */
int64_t itts_world_synth_length(int64_t n_frames, int fs, double frame_period_ms);

/* ---- host file I/O of the feature-extraction loop (no GPU; csrc/hostio.cpp) --------------------
 * AudioProcessing.get_raw (src/data_preparation/audio/AudioProcessing.py:107-120) for a batch:
 * mono PCM 8 / 16 / 32-bit or IEEE-float wav files -> float64 samples in [-1, 1] with
 * pre-emphasis raw[i] - p * raw[i-1], files read by n_threads threads.  Two passes: itts_wav_info
 * gives rate and length (ITTS_E_UNSUPPORTED for other layouts: read those another way), the caller
 * sizes one buffer, itts_wav_read_batch fills h_out[h_offsets[i] .. h_offsets[i+1]) with file i. */
int itts_wav_info(const char* h_path, int* fs, int64_t* n_samples);
int itts_wav_read_batch(const char* const* h_paths, int n_files, const int64_t* h_offsets,
                        double preemphasis, double* h_out, int n_threads);
/* The `.npz` archives save_output writes (world/WorldFeatLabelGen.py:1121-1172 through
 * LabelGen._save_to_npz, data_preparation/LabelGen.py:63-101) for a batch of utterances whose
 * features sit in one host matrix h_feat [Ttot, ld] f32 (utterance u = rows h_f_off[u] ..
 * h_f_off[u+1]): archive h_paths[u * n_streams + s] gets stream s = columns h_col0[s] ..., stored
 * as `<key>.npy` (h_parts[s] == 1, width h_width[s]) or as `<key>.npy`, `<key>_deltas.npy`,
 * `<key>_double_deltas.npy` (h_parts[s] == 3, three blocks of h_width[s] columns).  Archives are
 * written to `<path>_tmp` and renamed.  _save_to_npz keeps the other keys of an archive that already
 * exists: with h_needs_merge != NULL ([n_utts * n_streams] bytes) an existing archive holding
 * members this call would not write is left untouched and flagged 1 there (the caller merges it);
 * with NULL existing archives are replaced.  n_threads writer threads. */
int itts_write_feature_archives(const float* h_feat, int64_t ld, const int64_t* h_f_off, int n_utts,
                                const char* const* h_paths, int n_streams, const int* h_col0,
                                const int* h_width, const int* h_parts, const char* const* h_keys,
                                int n_threads, unsigned char* h_needs_merge);

/* Per-item normalisation of the data readers (NpzDataReader.preprocess_sample :347-371): h_out[r][c] =
 * (float)(((double)h_x[r][c] - h_sub[c]) / h_div[c]) -- numpy's `((x - sub) / div).astype(float32)` for float32 x and
 * float64 parameters, bit for bit, in one pass.  Host memory, no GPU. */
int itts_normalise_rows_f32(const float* h_x, int64_t rows, int cols, const double* h_sub,
                            const double* h_div, float* h_out);

/* ---- question labels (host, no GPU; csrc/labels.cpp) ------------------------------------------------
 * HTSLabelNormalisation (src/data_preparation/questions/label_normalisation.py): question-set
 * loading :817-897 (patterns compiled once per question), pattern matching :753-791,
 * load_labels_with_state_alignment :521-666.  Bit-identical to the reference.
 *   itts_questions_load      compiles a `.hed` question file (QS / CQS lines); *handle is freed with
 *                            itts_questions_free; label width = n_binary + n_continuous + 9
 *   itts_questions_vector    question answers of one context string -> h_out [n_binary + n_continuous]
 *   itts_labels_count_frames frames of every state-aligned `.lab` file (int((end - start) / 50000)
 *                            per state line; five state lines [2]..[6] per phone)
 *   itts_labels_generate     frame-level labels of all files into h_out [sum frames, ld_out] f64, file i at
 *                            rows h_frame_off[i] .. h_frame_off[i+1]: question vector of the phone +
 *                            the nine sub-phone features ('full'); files are spread over n_threads */
int itts_questions_load(const char* h_path, void** handle, int* n_binary, int* n_continuous);
void itts_questions_free(void* handle);
int itts_questions_vector(void* handle, const char* h_label, double* h_out);
int itts_labels_count_frames(const char* const* h_paths, int n_files, int64_t* h_frames, int n_threads);
int itts_labels_generate(void* handle, const char* const* h_paths, int n_files,
                         const int64_t* h_frame_off, double* h_out, int64_t ld_out, int n_threads);

/* ---- MLPG (misc/mlpg.py:94-127, bandmat solveh) ----------------------------------------- */
/*
 * Batched maximum-likelihood parameter generation with the reference's three windows
 * ([1], [-.5,0,.5], [1,-2,1]) for U utterances stored back to back.
 *   d_feat      [Ttot, ld_feat] f64; static/delta/delta-delta means of dimension d sit in
 *               columns col0+d, col0+D+d, col0+2D+d          (mlpg.py:119-121)
 *   d_var       [3*D] f64 diagonal of the 3D x 3D covariance (mlpg.py:111-113)
 *   h_offsets   [U+1] frame offsets of the utterances (host), offsets[U] = Ttot
 *   d_out       [Ttot, ld_out] f64; result for dimension d in column ocol0+d
 *   d_scratch   >= itts_mlpg_scratch_bytes(Ttot, D) bytes
 */
int64_t itts_mlpg_scratch_bytes(int64_t t_total, int dim);
int itts_mlpg_generation(const double* d_feat, int64_t ld_feat, int col0, int dim,
                         const double* d_var, const int64_t* h_offsets, int n_utts,
                         double* d_out, int64_t ld_out, int ocol0, void* d_scratch,
                         void* stream);
/* The same with float32 input rows -- the type the acoustic model's output has where mlpg.py:119-121 assigns it
 * into float64 arrays: the conversion happens in the solve's loads (exact), the result is that of
 * itts_mlpg_generation on the widened rows.   d_scratch >= itts_mlpg_scratch_bytes_f32(Ttot, D) bytes. */
int64_t itts_mlpg_scratch_bytes_f32(int64_t t_total, int dim);
int itts_mlpg_generation_f32(const float* d_feat, int64_t ld_feat, int col0, int dim,
                             const double* d_var, const int64_t* h_offsets, int n_utts,
                             double* d_out, int64_t ld_out, int ocol0, void* d_scratch,
                             void* stream);

/* A prepared plan for solving over the SAME utterance layout repeatedly -- the streams of one batch
 * (mlpg.py:94-127 is called once per stream: mcep, lf0, bap), a fixed validation set: the checks of the offsets,
 * the longest length and the one-pass kernel's (start, end) table in launch order are worked out once and kept
 * (the table in page-locked memory the launches read in place), so a planned call does nothing on the host but
 * launch.  The plan must outlive the work queued with it; destroy it after synchronising. */
int itts_mlpg_plan_create(const int64_t* h_offsets, int n_utts, void** plan_out);
void itts_mlpg_plan_destroy(void* plan);
int64_t itts_mlpg_plan_frames(const void* plan);
/* itts_mlpg_generation / itts_mlpg_generation_f32 (feat_is_f32) over the plan's utterances; d_scratch as for those. */
int itts_mlpg_generation_planned(const void* plan, const void* d_feat, int feat_is_f32, int64_t ld_feat, int col0,
                                 int dim, const double* d_var, double* d_out, int64_t ld_out, int ocol0,
                                 void* d_scratch, void* stream);

/* The form a call solves in, chosen from the batch's shape (all forms give the oracle's result to fp64 round-off):
 *   ITTS_MLPG_FORM_SWEEPS   longest utterance under 194 frames: the shared factor + one sequential sweep per
 *                           (utterance, dimension) (mlpg_factor_kernel, mlpg_kernel)
 *   ITTS_MLPG_FORM_STREAM   reduce -> scan -> solve over 16-frame chunks (mlpg_prep/reduce/scan/solve_kernel): from
 *                           194 frames with fewer than 128 (utterance, 64-dimension block) units, or more than
 *                           65 535 utterances
 *   ITTS_MLPG_FORM_RING     the one-pass kernel (mlpg_ring_kernel) otherwise
 * or-ed with
 *   ITTS_MLPG_FORM_WIDE          ring: two dimensions a lane in the helpers (float32 rows from 1 024 units, even D)
 *   ITTS_MLPG_FORM_F32_ROWS      float32 input rows
 *   ITTS_MLPG_FORM_NT_IN         ring, float64 rows, narrow: non-temporal input loads (rows of at most 192 MiB)
 *   ITTS_MLPG_FORM_WIDENED_COPY  float32 rows widened into a float64 copy first (mlpg_widen_kernel): every form but
 *                                the ring, which converts in its loads */
#define ITTS_MLPG_FORM_SWEEPS 1
#define ITTS_MLPG_FORM_STREAM 2
#define ITTS_MLPG_FORM_RING 3
#define ITTS_MLPG_FORM_SOLVE_MASK 3
#define ITTS_MLPG_FORM_WIDE 4
#define ITTS_MLPG_FORM_F32_ROWS 8
#define ITTS_MLPG_FORM_NT_IN 16
#define ITTS_MLPG_FORM_WIDENED_COPY 32
/* The form itts_mlpg_generation* would take for U = n_utts utterances of D = dim dimensions, the longest t_max frames,
 * t_total in all (float32 rows if rows_f32), under the current override.  No device work; -1 for bad sizes. */
int itts_mlpg_choose_form(int n_utts, int dim, int64_t t_max, int64_t t_total, int rows_f32);
/* Forces parts of the choice for every later call of the process (0 = the library's choice for that part):
 *   solve  ITTS_MLPG_FORM_STREAM or ITTS_MLPG_FORM_RING (batches under 194 frames keep the sweeps; forced ring
 *          with more than 65 535 utterances takes the stream form)
 *   width  ITTS_MLPG_FORCE_OFF (narrow) or ITTS_MLPG_FORCE_ON (wide; odd D stays narrow) -- ring only
 *   nt     ITTS_MLPG_FORCE_OFF or ITTS_MLPG_FORCE_ON -- ring with float64 rows, narrow, only
 * ITTS_E_INVALID for any other value.  The first use of the override seeds it from the environment:
 * ITTS_MLPG_RING / ITTS_MLPG_STREAM, ITTS_MLPG_NARROW / ITTS_MLPG_WIDE, ITTS_MLPG_NO_NT (set = forced). */
#define ITTS_MLPG_FORCE_OFF 1
#define ITTS_MLPG_FORCE_ON 2
int itts_mlpg_set_override(int solve, int width, int nt);
/* The override in force (any pointer may be NULL). */
int itts_mlpg_get_override(int* solve, int* width, int* nt);
/* The form (ITTS_MLPG_FORM_*) of the last itts_mlpg_generation* call on the calling thread; 0 when there was none,
 * or it had nothing to solve, or failed before choosing. */
int itts_mlpg_last_form(void);

/* The adjoint of the solve: the gradient of a loss with respect to the static / delta / delta-delta means, from its
 * gradient with respect to the trajectory.  For fixed variances the trajectory is linear in the means and P is
 * symmetric: z = P^-1 g (the same factor, g itself as the right-hand side), then the three windows,
 *   dL/dmu_0[t] = tau_0 z[t],  dL/dmu_1[t] = tau_1(t) 0.5 (z[t+1] - z[t-1]),  dL/dmu_2[t] = tau_2(t) (z[t-1] - 2 z[t] + z[t+1])
 * (z outside the utterance counts as 0; tau_w(t) = 1 / var_w, or 1e-11 in the first and last frame for w = 1, 2).
 *   d_gout      [Ttot, ld_gout] f64 (f32 if gout_is_f32): dL/dc of dimension d in column gcol0+d
 *   d_var, h_offsets (or the plan): as for itts_mlpg_generation
 *   d_gfeat     [Ttot, ld_gfeat] f64 (f32 if gfeat_is_f32): columns col0+d, col0+D+d, col0+2D+d of every frame are
 *               overwritten, nothing else is touched; arithmetic in f64, an f32 destination rounded once at the store
 *   d_scratch   >= itts_mlpg_adjoint_scratch_bytes(Ttot, D) bytes
 * Two forms, chosen per call as the forward chooses (no ring form):
 *   ITTS_MLPG_FORM_SWEEPS   longest utterance under 194 frames: mlpg_adjoint_kernel, one sequential sweep per
 *                           (utterance, dimension), the windows inside the back-substitution
 *   ITTS_MLPG_FORM_STREAM   from 194 frames: the forward's reduce -> scan -> solve over 16-frame chunks with the
 *                           gradient as the right-hand side, then one pointwise launch for the windows
 *                           (mlpg_adjoint_window_kernel); what it needs beyond d_scratch is the library's own
 *                           stream-ordered scratch
 * No atomics in either: repeated calls, planned or not, give identical bits (the two forms agree to rounding, not
 * bit for bit). */
int64_t itts_mlpg_adjoint_scratch_bytes(int64_t t_total, int dim);
int itts_mlpg_adjoint(const void* d_gout, int gout_is_f32, int64_t ld_gout, int gcol0, int dim,
                      const double* d_var, const int64_t* h_offsets, int n_utts,
                      void* d_gfeat, int gfeat_is_f32, int64_t ld_gfeat, int col0,
                      void* d_scratch, void* stream);
int itts_mlpg_adjoint_planned(const void* plan, const void* d_gout, int gout_is_f32, int64_t ld_gout, int gcol0,
                              int dim, const double* d_var, void* d_gfeat, int gfeat_is_f32, int64_t ld_gfeat,
                              int col0, void* d_scratch, void* stream);
/* The form (ITTS_MLPG_FORM_SWEEPS or ITTS_MLPG_FORM_STREAM) itts_mlpg_adjoint* would take for such a batch under the
 * adjoint's override.  No device work; -1 for bad sizes. */
int itts_mlpg_adjoint_choose_form(int n_utts, int dim, int64_t t_max, int64_t t_total);
/* Forces one form for every later adjoint call of the process, whatever the lengths: ITTS_MLPG_FORM_SWEEPS,
 * ITTS_MLPG_FORM_STREAM, or 0 for the library's choice; ITTS_E_INVALID for any other value.  A word of its own: the
 * forward's override (itts_mlpg_set_override) and itts_mlpg_last_form are not touched.  _get_override: the value in
 * force. */
int itts_mlpg_adjoint_set_override(int form);
int itts_mlpg_adjoint_get_override(void);
/* The form of the last itts_mlpg_adjoint* call on the calling thread; 0 when there was none, or it had nothing to
 * solve, or failed before choosing. */
int itts_mlpg_adjoint_last_form(void);

/* ---- frame utilities (misc/utils.py:40-105) --------------------------------------------- */
/* compute_deltas == np.gradient(x, axis=0) in float32 (utils.py:103-105): part of
 * itts_assemble_cmp_f32 below (static, delta, delta-delta columns of every stream in one pass). */

/* lf0 / V-UV of WorldFeatLabelGen.world_extract_features (world/WorldFeatLabelGen.py:798-802):
 *   lf0 = float32 log(clip(f0, 1e-10)); lf0[lf0 <= log(f0_silence_threshold)] = lf0_zero;
 *   lf0, vuv = interpolate_lin(lf0)
 * for U utterances stored back to back (h_f_off [U+1] frame offsets, each utterance < 2^24
 * frames).  d_f0 [Ttot] f64 -> d_lf0 [Ttot] f32 (interpolated, continuous), d_vuv [Ttot] f32. */
int itts_lf0_vuv(const double* d_f0, const int64_t* h_f_off, int n_utts,
                 double f0_silence_threshold, float lf0_zero, float* d_lf0, float* d_vuv,
                 void* stream);
/* d_x[i] = sqrt(d_x[i]) (IEEE, round to nearest): the amplitude envelope of
 * WorldFeatLabelGen.world_extract_features (world/WorldFeatLabelGen.py:795, np.sqrt(sp)) from CheapTrick's power
 * envelope, before it leaves the device. */
int itts_sqrt_inplace_f64(double* d_x, int64_t n, void* stream);
/* d_x[i] = d_x[i] * d_x[i] (one IEEE product): the power envelope WORLD's synthesis takes from the amplitude envelope
 * of WorldFeatLabelGen.world_features_to_raw (world/WorldFeatLabelGen.py:925, np.square), after the upload. */
int itts_square_inplace_f64(double* d_x, int64_t n, void* stream);

/* Short-time Fourier transform features (AudioProcessing.librosa_extract_amp_sp / extract_mfbanks,
 * AudioProcessing.py:156-226): librosa.stft of the float64 samples d_x (utterances back to back at
 * h_x_off [U+1]) with the window table d_window [n_fft] (scipy's window, zero-padded to n_fft and
 * centred), n_fft 1024 or 2048, hop > 0; pad_mode 0 = center=False, 1 = centre padding by np.pad
 * "reflect", 2 = "constant".  Output row g (h_f_off [U+1], h_f_off[0] = 0) of utterance u is STFT
 * frame g - h_f_off[u] + h_first[u] of that utterance (h_first drops frames in front: trim_to_shortest).
 * itts_stft writes |X| / sqrt(n_fft/2+1) to d_out [T, ld_out] as float32 (out_kind 0), float64 (1) or
 * 20 log10(max(1e-5, float32 value)) float32 (2).  itts_stft_mel writes the mel projection float32
 * [T, ld_out >= n_mels]: filter m sums d_mel_w[tab[3m+2] + j] * |X|[tab[3m] + j] / sqrt(K), j < tab[3m+1],
 * in ascending order (float64).  itts_mel_project applies the same tables to a given amplitude
 * spectrum d_amp [T, ld_amp] f64 with K bins.  Bit-identical from run to run. */
int itts_stft(const double* d_x, const int64_t* h_x_off, const int64_t* h_f_off, const int64_t* h_first,
              int n_utts, int n_fft, int hop, int pad_mode, const double* d_window, int out_kind,
              void* d_out, int64_t ld_out, void* stream);
int itts_stft_mel(const double* d_x, const int64_t* h_x_off, const int64_t* h_f_off, const int64_t* h_first,
                  int n_utts, int n_fft, int hop, int pad_mode, const double* d_window,
                  const int* d_mel_tab, const float* d_mel_w, int n_mels, float* d_out, int64_t ld_out,
                  void* stream);
int itts_mel_project(const double* d_amp, int64_t T, int K, int64_t ld_amp, const int* d_mel_tab,
                     const float* d_mel_w, int n_mels, float* d_out, int64_t ld_out, void* stream);

/* Griffin-Lim (librosa.griffinlim as AudioProcessing.amp_sp_to_raw, AudioProcessing.py:279-289, and
 * Synthesiser.run_griffin_lim / run_griffin_lim_on_log, Synthesiser.py:320-351, call it): n_iter iterations of
 * angles <- phase(stft(istft(S * angles)) - momentum / (1 + momentum) * previous stft) on the amplitude spectra
 * d_S [T, n_fft/2+1] of utterances stored back to back (rows h_f_off [U+1], h_f_off[0] = 0, >= 2 frames each),
 * then d_y = istft(S * angles), hop (T_u - 1) samples per utterance, back to back.  is_f64 = 0: d_S float32,
 * the phase state complex64 and d_y float32; 1: double / complex128 / double.  d_ang_a holds the initial
 * phases (overwritten); d_ang_b and d_tprev are workspaces of the same size.  d_window [n_fft]: the window
 * table (as for itts_stft); n_fft 1024 or 2048, 1 <= hop <= n_fft/2, pad_mode 1 (reflect) or 2 (constant) of
 * the centre padding.  One launch per iteration; bit-identical from run to run and whatever else is in the
 * batch.  itts_griffinlim_tile_frames: the frames per workgroup tile for (n_fft, hop), 0 when not covered. */
int itts_griffinlim(const void* d_S, void* d_ang_a, void* d_ang_b, void* d_tprev, const int64_t* h_f_off,
                    int n_utts, int n_fft, int hop, int pad_mode, const double* d_window, int n_iter,
                    double momentum, int is_f64, void* d_y, void* stream);
int itts_griffinlim_tile_frames(int n_fft, int hop);

/* Mel filter-bank inversion (librosa.feature.inverse.mel_to_stft(M, sr, n_fft, power=1.0, norm=None) times K, as
 * AudioProcessing.mfbanks_to_amp_sp, AudioProcessing.py:291-301, and decode_sp(sp_type="mfbanks"), :321-322,
 * call it): per frame b = row f of d_mel [n_frames, ld_mel] (float32, or double with mel_f64 = 1) the NNLS
 * problem min ||A x - b||^2, x >= 0, for the norm=None mel basis A [n_mels, K], K = n_fft / 2 + 1, solved by
 * FISTA with step inv_lipschitz = 1 / lambda_max(A A^T) from x = clip(pinv(A) b, 0), stopped every check_every
 * iterations once max |min(x, A^T (A x - b))| <= tol max |A^T b|, after max_iter iterations at the latest;
 * d_out row f [ld_out >= K] (float32, or double with out_f64 = 1) = K x.  The state is fp64.  Tables (built by
 * world.mel_inverse_tables), over KP = 64 ceil(K / 64) bins, zero beyond K: d_bin_j [KP] int32 m1 + 1 for the
 * two filters m1, m1 + 1 a bin lies in (0 .. n_mels), d_bin_w [KP][2] their weights, d_filt [n_mels][3] the bin
 * ranges [sb, eb) with m1 = m - 1 and [eb, ea) with m1 = m of filter m, d_pinv_t [n_mels, KP] pinv(A)^T.
 * d_iters [n_frames] (may be null): the iterations each frame took.  n_fft 1024 or 2048, 1 <= n_mels <= 256.
 * One wave per frame, one launch; bit-identical from run to run and whatever else is in the batch. */
int itts_mel_inverse(const void* d_mel, int64_t n_frames, int n_mels, int64_t ld_mel, int mel_f64, int n_fft,
                     const int* d_bin_j, const double* d_bin_w, const int* d_filt, const double* d_pinv_t,
                     double inv_lipschitz, double tol, int max_iter, int check_every, void* d_out, int64_t ld_out,
                     int out_f64, int* d_iters, void* stream);

/* interpolate_lin (misc/utils.py:40-86) on float32 contours stored back to back: frames <= 0 are
 * gaps; bit-exact including the reference's quirks (target reached one frame early; a gap whose
 * next voiced frame is the last frame is filled, with that frame, by the last voiced value).
 * d_ip [Ttot] f32 interpolated contour, d_vuv [Ttot] f32 (1 where d_in > 0).  In place
 * (d_ip == d_in) is allowed. */
int itts_interpolate_lin_f32(const float* d_in, const int64_t* h_off, int n_utts, float* d_ip,
                             float* d_vuv, void* stream);
/* Feature matrix of save_output / load (WorldFeatLabelGen.py:1121-1172, :459-573) for U utterances:
 * add_deltas != 0: [sp, d sp, dd sp | lf0, d, dd | vuv | bap, d bap, dd bap], width
 * 3*(n_sp+1+n_bap)+1 (the `.cmp` layout), d = compute_deltas = np.gradient in float32 per
 * utterance (misc/utils.py:103-105), dd = compute_deltas(d); else [sp | lf0 | vuv | bap].
 * d_sp [Ttot, ld_sp] f32, d_lf0 / d_vuv [Ttot] f32, d_bap [Ttot, ld_bap] f32 -> d_out [Ttot, ld_out]. */
int itts_assemble_cmp_f32(const float* d_sp, int64_t ld_sp, int n_sp, const float* d_lf0,
                          const float* d_vuv, const float* d_bap, int64_t ld_bap, int n_bap,
                          const int64_t* h_f_off, int n_utts, int add_deltas, float* d_out,
                          int64_t ld_out, void* stream);
/* Normalisation sums of MeanCovarianceExtractor / MeanStdDevExtractor.add_sample
 * (misc/normalisation/MeanCovarianceExtractor.py:27-31, MeanStdDevExtractor.py) over columns
 * [col0, col0+width) of d_x [n_rows, ld_x] f32, accumulated in fp64 with a fixed summation order:
 * d_sum [width] = sum x; d_second = sum x x^T [width, width] (want_cov != 0; fp64 matrix cores)
 * or sum x^2 [width].  accumulate != 0 adds to the outputs.
 * d_workspace >= itts_feature_stats_workspace_bytes(width, want_cov). */
int64_t itts_feature_stats_workspace_bytes(int width, int want_cov);
int itts_feature_stats(const float* d_x, int64_t ld_x, int64_t n_rows, int col0, int width,
                       int want_cov, int accumulate, double* d_sum, double* d_second,
                       void* d_workspace, void* stream);

/* Row gather of the recurrent layers' packed layout -- pack_padded_sequence / pad_packed_sequence and
 * their gradients (rnn_dyn/RNNWrapper.py:89-102), and the h_{t-1} shift of the weight gradient:
 * d_dst[r, :width] = d_src[d_idx[r], :width] where 0 <= d_idx[r] < n_src, else d_fill_row[:width] (zeros when
 * NULL); columns width .. dst_width - 1 of every row of d_dst are zeroed (16-byte row pitches for the GEMMs). */
int itts_rows_gather_f32(const float* d_src, int64_t ld_src, int64_t n_src, const int64_t* d_idx, int64_t n_out,
                         int width, const float* d_fill_row, float* d_dst, int64_t ld_dst, int dst_width,
                         void* stream);

/* ---- mini-batches on the device (ModularModelHandlerPyTorch.prepare_batch :388-465, sequence_mask :467-491) ----
 * The rows of the utterances of a batch lie back to back in d_src (utterance b: rows d_starts[b] .. d_starts[b] +
 * d_lens[b] - 1, d_starts / d_lens on the device); the padded batch is [n_utts, t_max, width] (batch_first) or
 * [t_max, n_utts, width] with row pitch ld_dst.  Position (b, t) receives row d_starts[b] + t for t < d_lens[b]
 * (and a row inside [0, n_src)), else d_fill_row[:width] (zeros when NULL) -- pad_sequence of the cached rows, or
 * pad_packed_sequence with the layers' value of a padding position as the fill row; the padding position with flat
 * index rep_pos (in the batch's layout; -1: none) receives d_rep_row[:width] instead; d_mask (may be NULL) receives
 * the float sequence mask, one value per position in the batch's layout. */
int itts_batch_pad_gather_f32(const float* d_src, int64_t ld_src, int64_t n_src, const int64_t* d_starts,
                              const int64_t* d_lens, int n_utts, int64_t t_max, int width, int batch_first,
                              const float* d_fill_row, int64_t rep_pos, const float* d_rep_row, float* d_dst,
                              int64_t ld_dst, float* d_mask, void* stream);
/* The adjoint: d_dst[d_starts[b] + t, :width] = padded position (b, t) of d_src for t < d_lens[b]; columns width ..
 * dst_width - 1 of the written rows are zeroed (16-byte row pitches for the GEMMs).  Padding positions are not read,
 * except the one with flat index rep_pos (-1: none), which is written to row rep_dst_row. */
int itts_batch_pack_rows_f32(const float* d_src, int64_t ld_src, const int64_t* d_starts, const int64_t* d_lens,
                             int n_utts, int64_t t_max, int width, int batch_first, float* d_dst, int64_t ld_dst,
                             int dst_width, int64_t rep_pos, int64_t rep_dst_row, void* stream);
/* d_dst[d_dst_starts[b] + t, :width] = d_src[d_src_starts[b] + t, :width] for t < d_lens[b] (t_max >= every length);
 * columns width .. dst_width - 1 of the written rows are zeroed: the valid frames of a mini-batch's utterances out of
 * an arena, back to back in batch order -- the packed batch of the flat feed-forward step
 * (data_preparation/FrameShard.py: gather), one launch instead of a row index built on the host. */
int itts_batch_concat_rows_f32(const float* d_src, int64_t ld_src, int64_t n_src, const int64_t* d_src_starts,
                               const int64_t* d_dst_starts, const int64_t* d_lens, int n_utts, int64_t t_max, int width,
                               float* d_dst, int64_t ld_dst, int dst_width, void* stream);
/* d_out[c] = sum of d_x[(b, t), c] over the padding positions (t >= d_lens[b]) of a padded batch, summed in a fixed
 * order (the gradient that reaches the fill row of itts_batch_pad_gather_f32); d_out[width .. out_width - 1] = 0.
 * d_workspace: itts_batch_pad_colsum_workspace_bytes(n_utts * t_max, width) bytes on the device. */
int64_t itts_batch_pad_colsum_workspace_bytes(int64_t n_rows, int width);
int itts_batch_pad_colsum_f32(const float* d_x, int64_t ld_x, const int64_t* d_lens, int n_utts, int64_t t_max,
                              int width, int batch_first, float* d_out, int out_width, void* d_workspace,
                              void* stream);

/* ---- acoustic model: dense layers (rnn_dyn/FFWrapper.py:63-73 -> torch.nn.Linear + act) --- */
/* Activation codes (act / act_prev): the torch.nn module of that name with its default arguments.
 * The backward derives act' from the layer OUTPUT y (no pre-activation is stored); at a branch point
 * it takes torch's value.  The Conv1d entry points below accept NONE, TANH and RELU only.
 *   code  module        y = f(z)                            act'(y)
 *   0     (none)        z                                   1
 *   1     Tanh          tanh z                              1 - y^2
 *   2     ReLU          max(z, 0)                           y > 0
 *   3     Sigmoid       1 / (1 + e^-z)                      y (1 - y)
 *   4     LogSigmoid    min(z, 0) - log1p(e^-|z|)           -expm1(y)
 *   5     Softplus      z > 20 ? z : log1p(e^z)             y > 20 ? 1 : -expm1(-y)
 *   6     Softsign      z / (1 + |z|)                       (1 - |y|)^2
 *   7     LeakyReLU     z > 0 ? z : 0.01 z                  y > 0 ? 1 : 0.01
 *   8     ELU           z > 0 ? z : expm1(z)                y > 0 ? 1 : y + 1
 *   9     CELU          as ELU (alpha 1)                    as ELU
 *   10    SELU          s (z > 0 ? z : a expm1(z))          y > 0 ? s : y + s a   (torch's a, s)
 *   11    Hardtanh      clamp(z, -1, 1)                     -1 < y < 1
 *   12    ReLU6         clamp(z, 0, 6)                      0 < y < 6
 *   13    Hardsigmoid   clamp(z + 3, 0, 6) / 6              0 < y < 1 ? 1/6 : 0 */
#define ITTS_ACT_NONE 0
#define ITTS_ACT_TANH 1
#define ITTS_ACT_RELU 2
#define ITTS_ACT_SIGMOID 3
#define ITTS_ACT_LOGSIGMOID 4
#define ITTS_ACT_SOFTPLUS 5
#define ITTS_ACT_SOFTSIGN 6
#define ITTS_ACT_LEAKY_RELU 7
#define ITTS_ACT_ELU 8
#define ITTS_ACT_CELU 9
#define ITTS_ACT_SELU 10
#define ITTS_ACT_HARDTANH 11
#define ITTS_ACT_RELU6 12
#define ITTS_ACT_HARDSIGMOID 13
/* Pitch rule for the row-major activations of the four entry points below (x, y, dz, dx, yprev):
 * a row pitch (ld*) that is a multiple of 4 floats on a 16-byte aligned base selects 16-byte loads.
 * If the logical width is not a multiple of 4, the 1-3 floats between the width and the next
 * multiple of 4 are then read as well and must be finite (keep them zero): a padded reduction
 * element meets a zero of the other operand.  Of an output with such rows the same 1-3 floats are either left
 * alone (the register-staged kernel) or written as zeros (the ring kernel); no call writes anything else outside
 * its [M, width] slice, so outputs may be column slices of wider buffers.
 * y[M,N] = act(x[M,K] @ w[N,K]^T + b[N]); fp32 MFMA. */
int itts_linear_fwd(const float* d_x, int64_t ldx, const float* d_w, const float* d_b,
                    float* d_y, int64_t ldy, int64_t M, int N, int K, int act, void* stream);
/* Output layer of a training step fused with NamedLoss(MSELoss, reduction 'mean_per_frame')
 * (FFWrapper.py:63-73 + loss/NamedLoss.py:70-117): y = x w^T + b is never stored; d_loss [1] receives
 * loss_weight * sum_valid (y - target)^2 / (n_valid * N) and d_dz [M, N] its gradient w.r.t. y.
 * x, w and dz need 16-byte aligned rows (ldx, K, lddz multiples of 4); d_workspace:
 * itts_linear_fwd_mse_workspace_bytes(M, N) bytes. */
int64_t itts_linear_fwd_mse_workspace_bytes(int64_t M, int N);
int itts_linear_fwd_mse(const float* d_x, int64_t ldx, const float* d_w, const float* d_b,
                        const float* d_target, int64_t ldt, const uint8_t* d_row_valid, double n_valid,
                        float loss_weight, int64_t M, int N, int K, float* d_loss, float* d_dz,
                        int64_t lddz, void* d_workspace, void* stream);

/* dz = dy * act'(y)  (elementwise; act' expressed through the layer output y). */
int itts_act_bwd(const float* d_dy, const float* d_y, float* d_dz, int64_t n_elem, int act,
                 void* stream);
/* dx[M,K] = dz[M,N] @ w[N,K]; if d_yprev != NULL the previous layer's act' (through its
 * output yprev[M,K]) is fused into the epilogue: dx *= act'(yprev). */
int itts_linear_bwd_input(const float* d_dz, int64_t lddz, const float* d_w, float* d_dx,
                          int64_t lddx, const float* d_yprev, int64_t ldyp, int act_prev,
                          int64_t M, int N, int K, void* stream);
/* dw[N,K] = dz[M,N]^T @ x[M,K], db[N] = colsum(dz).  Deterministic split-K through
 * d_workspace (>= itts_linear_bwd_weight_workspace_bytes). If accumulate != 0, adds. */
int64_t itts_linear_bwd_weight_workspace_bytes(int64_t M, int N, int K);
int itts_linear_bwd_weight(const float* d_dz, int64_t lddz, const float* d_x, int64_t ldx,
                           float* d_dw, float* d_db, int64_t M, int N, int K,
                           void* d_workspace, int accumulate, void* stream);
/* Both gradients of a layer from dz in one call (autograd's backward of torch.nn.Linear in
 * rnn_dyn/FFWrapper.py:63-73): dw / db as itts_linear_bwd_weight, dx as itts_linear_bwd_input
 * (d_yprev != NULL: times the derivative of the previous layer's activation).  With 16-byte rows
 * the two GEMMs share one launch; the results equal the separate calls bit for bit.  d_workspace
 * as for itts_linear_bwd_weight. */
int itts_linear_bwd(const float* d_dz, int64_t lddz, const float* d_x, int64_t ldx, const float* d_w,
                    float* d_dw, float* d_db, float* d_dx, int64_t lddx, const float* d_yprev,
                    int64_t ldyp, int act_prev, int64_t M, int N, int K, void* d_workspace,
                    int accumulate, void* stream);

/* ---- dropout fused into the dense layers (csrc/dropout.h; replaces the nn.Dropout behind every layer of a Linear
 * group, rnn_dyn/FFWrapper.py:40-61) ---------------------------------------------------------------------------
 * The mask is a function of the element's position, not of a generator's state, so a backward recomputes it and
 * none is stored.  Element (row, col) of a matrix, with a 64-bit seed, a 32-bit salt, a probability p in [0, 1) and
 * an int64 row_offset: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (r & 0xffffffff, r >> 32,
 * col >> 2, salt), r = row + row_offset; output word col & 3 keeps the element iff word >= min(2^32 - 1,
 * round(p * 2^32)).  Kept elements are multiplied by scale = 1 / (1 - p) (float32 of 1 - p, float32 division);
 * dropped elements are +0.0.  Every entry point below with p == 0 launches exactly what its counterpart without the
 * suffix launches.
 *
 * out = in * m * scale on [M, N] rows with pitches ldi / ldo (floats), forward and backward alike; d_out may be d_in.
 * mask_only != 0: d_out is uint8 [M, ldo] and receives m itself (1 kept, 0 dropped); d_in is not read. */
int itts_dropout_apply(const float* d_in, int64_t ldi, void* d_out, int64_t ldo, int64_t M, int N, int mask_only,
                       double p, uint64_t seed, uint32_t salt, int64_t row_offset, void* stream);
/* dz = dy * m * scale * act'(y), y = d * (1 - p): back through the dropout and the activation of a layer from its
 * dropped output d [M, ldd] (itts_act_bwd for such a layer); d_dz may be d_dy. */
int itts_dropout_act_bwd(const float* d_dy, int64_t lddy, const float* d_d, int64_t ldd, float* d_dz, int64_t lddz,
                         int64_t M, int N, int act, double p, uint64_t seed, uint32_t salt, int64_t row_offset,
                         void* stream);
/* itts_linear_fwd with the rule on the output: y = act(x w^T + b) * m * scale. */
int itts_linear_fwd_dropout(const float* d_x, int64_t ldx, const float* d_w, const float* d_b, float* d_y, int64_t ldy,
                            int64_t M, int N, int K, int act, double p, uint64_t seed, uint32_t salt,
                            int64_t row_offset, void* stream);
/* itts_linear_bwd_input where the previous layer's output d_yprev [M, ldyp] (required) carries the rule (p, seed,
 * salt, row_offset): dx = (dz w) * m * scale * act_prev'(y), y = d_yprev * (1 - p) where m = 1. */
int itts_linear_bwd_input_dropout(const float* d_dz, int64_t lddz, const float* d_w, float* d_dx, int64_t lddx,
                                  const float* d_yprev, int64_t ldyp, int act_prev, int64_t M, int N, int K, double p,
                                  uint64_t seed, uint32_t salt, int64_t row_offset, void* stream);
/* itts_linear_bwd with the input gradient of itts_linear_bwd_input_dropout (dw / db need nothing new: dz and x are
 * the dropped values already); equal to the separate calls bit for bit. */
int itts_linear_bwd_dropout(const float* d_dz, int64_t lddz, const float* d_x, int64_t ldx, const float* d_w,
                            float* d_dw, float* d_db, float* d_dx, int64_t lddx, const float* d_yprev, int64_t ldyp,
                            int act_prev, int64_t M, int N, int K, void* d_workspace, int accumulate, double p,
                            uint64_t seed, uint32_t salt, int64_t row_offset, void* stream);
/* itts_linear_fwd_sparse (below) with the rule on the output. */
int itts_linear_fwd_sparse_dropout(const void* d_lists, const float* d_x, int64_t ldx, const float* d_w,
                                   const float* d_b, float* d_y, int64_t ldy, int64_t M, int N, int K, int act,
                                   double p, uint64_t seed, uint32_t salt, int64_t row_offset, void* stream);

/* ---- dense layer on a sparse input (the min-max-normalised question vectors of layer 0: binary answers, mostly
 * exact zeros) -------------------------------------------------------------------------------------------------
 * Row lists of x [M, ldx]: per row the (k, x[m,k]) pairs with x[m,k] != 0 in ascending k (+-0.0 dropped; NaN and
 * denormals kept; columns >= K never listed), K <= 65535.  They live in ONE caller-owned block d_lists whose layout
 * itts_sparse_rows_layout gives: out = {byte offset of the int32 counts [M], byte offset of the entries
 * [M][pitch] of {int32 k, float value}, pitch in entries, size of the block in bytes}.  Bytes 0..15 of the block
 * are the record {int64 total non-zeros, int64 largest count of a row}, written only when want_record != 0 (one
 * more memset; a caller that has decided leaves it out).  A row of K non-zeros gives K entries: nothing is capped.
 * No float atomics, no host synchronisation. */
int itts_sparse_rows_layout(int64_t M, int K, int64_t out[4]);
int itts_sparse_rows_build(const float* d_x, int64_t ldx, int64_t M, int K, void* d_lists, int want_record,
                           void* stream);
/* y[M,N] = act(b[N] + sum over the listed (k, v) of row m of v * w[n,k]) with d_lists built from x [M, K]: one fmaf
 * chain per output in ascending k, starting from +0, the bias added last; activations and the pad columns of y
 * as itts_linear_fwd (written as zeros where that writes them).  Each workgroup keeps a 64-column slab of w^T in
 * LDS, which holds K <= 512; a larger K runs itts_linear_fwd on d_x instead (decided from the shape alone), so
 * d_x / ldx must be the matrix the lists were built from. */
int itts_linear_fwd_sparse(const void* d_lists, const float* d_x, int64_t ldx, const float* d_w, const float* d_b,
                           float* d_y, int64_t ldy, int64_t M, int N, int K, int act, void* stream);
/* Process-wide atomic counts, no device call: out = {itts_sparse_rows_build launches, itts_linear_fwd_sparse calls
 * that ran the sparse kernel, itts_linear_fwd_sparse calls that ran the dense product instead}. */
int itts_sparse_path_counts(int64_t out[3]);

/* Weight gradient of the same layer, dw[N][lddw] = dz^T x (+ db[N] = column sums of dz), without the products by
 * x's zeros (csrc/sparse_wgrad.hip).  The non-zeros are walked by column, K <= 512 and lddw <= 512.
 * Plan (d_plan, itts_sparse_cols_plan_ints() = 1056 int32 on the device): plan[0..30] are the heavy columns of x
 * (-1: none; plan[31] is ignored, that strip column is the ones of the bias), plan[32 + 8 o + s] is the light column
 * in slot s of owner o (64 owners, -1: none), and plan[544 + k] says the same from column k's side: 8 o + s, or
 * 0x1000 + h for the heavy column in strip column h.  Every column < K must stand in it exactly once.  Which column
 * is heavy and who owns a light one only moves time: any such plan gives the same sums up to their order.
 * Column data of one batch (itts_sparse_cols_build into the caller-owned, 16-byte aligned block d_cols;
 * itts_sparse_cols_layout: out = {byte offset of the strip, byte offset of the streams, size in bytes}): x is cut into
 * tiles of 256 rows; the strip float [tiles * 256][32] holds the heavy columns' values (column 31: 1.0, rows behind M:
 * 0); the streams are uint16 counts[tiles * 64][8], then block 0 of every list, [tiles * 64 * 8][16] entries, then
 * blocks 1..15 of every list, [tiles * 64 * 8][15][16] entries, list (tile * 64 + owner) * 8 + slot; an entry is {int32
 * byte offset of the row in a [257][64] float tile, float value}, rows ascending, the last block of a list filled
 * up with {row 256, +0.0}.  -0.0 / NaN / denormals as in
 * itts_sparse_rows_build; a column of 256 non-zeros gives 256 entries: nothing is capped.
 * itts_sparse_cols_build_from_rows writes the same block from the row lists d_lists of the same x
 * (itts_sparse_rows_build over K_lists >= K columns; listed columns >= K are left out) without reading x: the same
 * counts, the same entries in the same order, the same strip -- but for a -0.0 in a heavy column, which the lists do
 * not hold: its strip cell is +0.0 where the build from x copies the sign bit (no sum depends on it).
 * itts_linear_bwd_weight_sparse: the result goes through the split-K slab workspace and the reduction of
 * itts_linear_bwd_weight (itts_defer_reductions applies, accumulate likewise; workspace size from the _sparse query);
 * dw's pad columns K..lddw-1 become zeros.  Deterministic, no float atomics: a light column's fmaf chain runs in
 * ascending m per row range, a heavy column's per wave share, the shares in wave order, the ranges in slab order.
 * What the kernel does not serve -- K or lddw > 512, lddz % 4 != 0, dz or d_cols not 16-byte aligned, d_plan or
 * d_cols NULL -- runs itts_linear_bwd_weight on d_x over lddw columns instead (decided on the host; then lddw == K,
 * or ldx >= lddw with x's pad columns zero).  itts_sparse_wgrad_counts: out = {column build launches (either entry),
 * calls that ran the sparse kernel, calls that ran the dense product}; process-wide, no device call. */
int itts_sparse_cols_plan_ints(void);
int itts_sparse_cols_layout(int64_t M, int K, int64_t out[3]);
int itts_sparse_cols_build(const float* d_x, int64_t ldx, int64_t M, int K, const int* d_plan, void* d_cols,
                           void* stream);
int itts_sparse_cols_build_from_rows(const void* d_lists, int64_t M, int K_lists, int K, const int* d_plan,
                                     void* d_cols, void* stream);
int64_t itts_linear_bwd_weight_sparse_workspace_bytes(int64_t M, int N, int K, int64_t lddw);
int itts_linear_bwd_weight_sparse(const float* d_dz, int64_t lddz, const void* d_cols, const int* d_plan,
                                  const float* d_x, int64_t ldx, float* d_dw, int64_t lddw, float* d_db, int64_t M,
                                  int N, int K, void* d_workspace, int accumulate, void* stream);
int itts_sparse_wgrad_counts(int64_t out[3]);

/* ---- acoustic model: Conv1d groups (rnn_dyn/CNNWrapper.py:28-61 -> torch.nn.Conv1d + act) ---
 * 1-D convolution over the time axis of a zero-padded batch of B utterances, stride 1, groups 1,
 * padding_mode 'zeros': T_out = T_in + 2 pad - dil (Kw - 1) (> 0, else ITTS_E_INVALID).  Activations
 * are rows: row (b, t) is b * T + t (batch_first != 0) or t * B + b (time-major), T = T_in for x /
 * dx / yprev and T_out for y / dz.  A time index outside [0, T_in) counts as zero (the edge of the
 * padded tensor, not the valid length: nn.Conv1d on the padded batch).  w is torch's
 * [Cout][Cin][Kw], contiguous.  fp32 MFMA implicit GEMM (the im2col matrix is never stored); the
 * pitch rule of the dense layers above applies to x, dz and their 1-3 pad floats.
 * y[(b,t), n] = act(b[n] + sum_k sum_c x[(b, t + k dil - pad), c] w[n][c][k])  (d_b may be NULL). */
int itts_conv1d_fwd(const float* d_x, int64_t ldx, const float* d_w, const float* d_b, float* d_y,
                    int64_t ldy, int B, int T_in, int Cin, int Cout, int Kw, int pad, int dil,
                    int batch_first, int act, void* stream);
/* Autograd's input gradient of nn.Conv1d (CNNWrapper.py:55-61 backward): dx [B*T_in, Cin] from dz
 * [B*T_out, Cout]; if d_yprev != NULL the previous layer's act' (through its output yprev, rows as
 * dx) is fused into the epilogue: dx *= act'(yprev). */
int itts_conv1d_bwd_input(const float* d_dz, int64_t lddz, const float* d_w, float* d_dx, int64_t lddx,
                          const float* d_yprev, int64_t ldyp, int act_prev, int B, int T_in, int Cin,
                          int Cout, int Kw, int pad, int dil, int batch_first, void* stream);
/* dw[n][c][k] = sum_(b,t) dz[(b,t), n] x[(b, t + k dil - pad), c], db[n] = colsum(dz) (d_db may be
 * NULL): nn.Conv1d's weight / bias gradients.  Deterministic split over the B*T_out rows through
 * d_workspace (>= itts_conv1d_bwd_weight_workspace_bytes); bit-identical run to run.  If
 * accumulate != 0, adds. */
int64_t itts_conv1d_bwd_weight_workspace_bytes(int B, int T_in, int Cin, int Cout, int Kw, int pad, int dil);
int itts_conv1d_bwd_weight(const float* d_dz, int64_t lddz, const float* d_x, int64_t ldx, float* d_dw,
                           float* d_db, int B, int T_in, int Cin, int Cout, int Kw, int pad, int dil,
                           int batch_first, void* d_workspace, int accumulate, void* stream);
/* What such a call runs, without device work (the function the three entry points take their choice
 * from): product 0 = itts_conv1d_fwd, 1 = _bwd_input, 2 = _bwd_weight; vec != 0 when the operands
 * allow 16-byte loads (pitch % 4 == 0 and a 16-byte aligned base, of x for 0, dz for 1, both for 2).
 * *tile_cols: 64 or 128 output columns per workgroup tile; *slabs: parts of the reduction summed in
 * a fixed order (1 except for the weight gradient); *kchunk: reduction elements per slab (a multiple
 * of 32; the last slab may hold fewer).  Any of the three may be NULL.  Returns 0, or -1 for an
 * unknown product or a geometry the entry points reject. */
int itts_conv1d_plan(int product, int B, int T_in, int Cin, int Cout, int Kw, int pad, int dil, int vec,
                     int* tile_cols, int* slabs, int64_t* kchunk);

/* ---- LayerNorm layer groups (rnn_dyn/FFWrapper.py: torch.nn.LayerNorm(normalized_shape=D) + the group's
 *      non-linearity; csrc/layernorm.hip) --------------------------------------------------------
 * y[N,D] = act((x - mean) * rstd * gamma + beta) per row: mean and the biased variance over the row's D
 * columns (two passes, on the centred values), rstd = 1 / sqrt(var + eps); d_mean / d_rstd [N] receive
 * them for the backward.  d_gamma / d_beta [D] may each be NULL (elementwise_affine=False, bias=False);
 * act is any ITTS_ACT_* code.  1 <= D <= 4096, anything wider is refused before any device work.
 * Row pitches ld* >= D; pitches that are multiples of 4 floats on 16-byte aligned bases select 16-byte
 * loads and stores (whatever lies between D and the pitch is read and dropped, never written).  A row's
 * result depends on nothing but the row: the same bits for any N, any position and either load form. */
int itts_layernorm_fwd(const float* d_x, int64_t ldx, const float* d_gamma, const float* d_beta,
                       float* d_y, int64_t ldy, float* d_mean, float* d_rstd, int64_t N, int D,
                       double eps, int act, void* stream);
/* With dy' = dy * act'(y) (through the forward's output y; d_y may be NULL for ITTS_ACT_NONE),
 * g = dy' * gamma and xhat = (x - mean) * rstd:
 *   dx = rstd * (g - mean_D(g) - xhat * mean_D(g * xhat)),  dgamma = sum_rows dy' * xhat,  dbeta = sum_rows dy'.
 * d_dgamma / d_dbeta [D] may each be NULL; when either is given, d_workspace holds
 * itts_layernorm_workspace_bytes(N, D) bytes: one slab of 2 * D floats per workgroup of
 * 32 * ceil(N / 32768) rows, summed in a fixed order by a second launch (no atomics: repeated calls give
 * identical bits). */
int64_t itts_layernorm_workspace_bytes(int64_t N, int D);
int itts_layernorm_bwd(const float* d_dy, int64_t lddy, const float* d_x, int64_t ldx,
                       const float* d_y, int64_t ldy, const float* d_mean, const float* d_rstd,
                       const float* d_gamma, float* d_dx, int64_t lddx, float* d_dgamma,
                       float* d_dbeta, int64_t N, int D, int act, void* d_workspace, void* stream);

/* ---- multi-head self-attention (torch.nn.MultiheadAttention inside torch.nn.TransformerEncoderLayer, which the
 *      reference reaches through rnn_dyn/FFWrapper.py:62-73; csrc/attention.hip) ---------------------------------
 * o = softmax(q k^T * scale) v per utterance b and head h, all float32, without a [T, T] tensor in global memory
 * (online softmax over key tiles of 32).  d_qkv [rows, 3 D] holds q | k | v per row as the in-projection writes
 * it, head h in columns h * dh .. (h + 1) * dh of each third, D = H * dh; d_o [rows, D].  Row of (b, t) =
 * b * stride_b + t * stride_t, so [B, T, .] (stride_b = T, stride_t = 1) and [T, B, .] (1, B) both work.
 * d_klen [B] (int32, device): query t of utterance b attends keys 0 .. klen[b] - 1, for EVERY t < T;
 * 1 <= klen[b] <= T (not checked on the device: a larger value is clamped to T, a smaller one to 1).  Rows of
 * k / v at and beyond klen[b] are never used (they may hold NaN).  NULL d_klen: klen = T.  scale = 1 / sqrt(dh).
 * d_lse [B, H, T] (itts_attention_workspace_bytes) receives ln sum_k exp(score) per query for the backward.
 * p > 0: dropout on the softmax probabilities before P v (DropRule of csrc/dropout.h: key = seed, salt = salt),
 * element (row = (b * H + h) * T + t, col = key): the mask depends on b, h, t and T, so utterances of a batch
 * draw independent masks, as in torch; p == 0 runs the kernel without a generator.
 * The order of every sum depends on klen[b] and the tile sizes only: the same bits for any B, T and position.
 * Envelope (else ITTS_E_INVALID before any device work): dh a multiple of 4 in 4 .. 128 (computed at
 * the next multiple of 32), D <= 1024,
 * 1 <= T <= 32768, B * H <= 65535, strides >= 1; B == 0 succeeds and does nothing. */
int64_t itts_attention_workspace_bytes(int B, int H, int T);
int itts_attention_fwd(const float* d_qkv, float* d_o, const int32_t* d_klen, float* d_lse, int B, int T, int H,
                       int dh, int64_t stride_b, int64_t stride_t, double p, uint64_t seed, uint32_t salt,
                       void* stream);
/* d_dqkv [rows, 3 D] = (dq | dk | dv) from d_do [rows, D], the forward's d_qkv, d_o and d_lse and the same rule.
 * Every element of the B * T addressed rows is written exactly once (dk / dv rows at and beyond klen[b]: zero).
 * P is recomputed from q, k and the log-sum-exp; the mask is recomputed.  Three launches: delta = rowsum(do * o);
 * dk / dv, one workgroup per 128 keys sweeping the query tiles; dq, one workgroup per 128 queries sweeping the key
 * tiles.  No atomics and no waiting between workgroups: repeated calls give identical bits. */
int itts_attention_bwd(const float* d_do, const float* d_qkv, const float* d_o, const int32_t* d_klen,
                       const float* d_lse, float* d_dqkv, int B, int T, int H, int dh, int64_t stride_b,
                       int64_t stride_t, double p, uint64_t seed, uint32_t salt, void* stream);

/* ---- all-pass frequency warping, the VTLN layer (csrc/allpass.hip) ------------------------------------------
 * Rows of D = nb * N floats are nb blocks of N cepstral coefficients, each warped by the row's own factor:
 * y_b = x_b' W(alpha), W the N x N all-pass matrix of the recursion W[0][0] = 1, W[0][c] = 0,
 * W[r][0] = alpha W[r-1][0], W[r][c] = W[r-1][c-1] + alpha (W[r-1][c] - W[r][c-1]), applied inside the kernel
 * (no matrix is stored).  In blocks 0..2 the first coefficient is halved before and doubled after.  With d_mean /
 * d_std_dev [D] (each may be NULL) the input is first taken as x * std_dev + mean and the output written as
 * (y - mean) / std_dev.  1 <= N <= 64, D a multiple of N, row pitches >= D; anything else is refused with
 * ITTS_E_INVALID and a message naming the value before any device work; M == 0 succeeds and does nothing.
 * d_x is never written.
 * Reference: layers/AllPassWarp.py:148-173 (AllPassWarp.forward) inside layers/AllPassWarpLayer.py:141-150
 * (forward_fixed_alphas: _denormalise, warp, _normalise). */
int itts_allpass_warp_fwd(const float* d_x, int64_t ldx, const float* d_alpha, const float* d_mean,
                          const float* d_std_dev, float* d_y, int64_t ldy, int64_t M, int D, int N,
                          void* stream);
/* Gradients of the above for d_dy = dL/dy: d_dx [M, D] and d_dalpha [M].  W and dW/dalpha are recomputed from
 * alpha (only x and alpha are needed from the forward); a row's dalpha is summed by the lane that owns the row,
 * in a fixed order and without atomics, so repeated calls give identical bits.
 * Reference: autograd through layers/AllPassWarp.py:157-171 (get_warp_matrix's einsum and the bmm). */
int itts_allpass_warp_bwd(const float* d_dy, int64_t lddy, const float* d_x, int64_t ldx,
                          const float* d_alpha, const float* d_mean, const float* d_std_dev, float* d_dx,
                          int64_t lddx, float* d_dalpha, int64_t M, int D, int N, void* stream);

/* ---- utterance-level latents: time pooling, VAE reparameterisation, KL term (csrc/latent.hip) ----------------
 * All float32; row pitches in floats; 16-byte loads when a pitch is a multiple of 4 floats and its base is 16-byte
 * aligned, plain loads otherwise (the same bits either way).  Every refusal is ITTS_E_INVALID with a message that
 * names the value, before any device work; empty calls (n_utts == 0, M == 0) succeed.  No float atomics: repeated
 * calls give identical bits.
 *
 * Pooling of a padded batch over time: d_x is [n_utts, t_max, width] (batch_first != 0) or [t_max, n_utts, width],
 * position pitch ldx, d_y [n_utts, width] with pitch ldy; d_lens int64 [n_utts] on the device, as for
 * itts_batch_pad_gather_f32.
 *   ITTS_POOL_LAST  y[b] = x[b, len_b - 1], the row index clamped into [0, t_max); d_lens == NULL: row t_max - 1.
 *   ITTS_POOL_MEAN  y[b] = (sum of ALL t_max positions of x[b], padding included) / len_b; d_lens == NULL is
 *                   refused.  After a recurrent group the padding is zero and this is the masked mean; after
 *                   Linear groups it is not (the reference divides the plain sum the same way).
 * An utterance's result depends on its own rows, t_max and the layout only, never on its batch index or on n_utts:
 * time is summed in segments of 128 rows in one fixed order.  With few (utterance, 256-column tile) pairs every
 * segment gets a workgroup and a second launch adds the segment sums from d_workspace in that same order;
 * itts_time_pool_plan says, without device work, how many segments a shape has, whether the call is split that way
 * and how many workspace bytes it then needs (0 otherwise; d_workspace may be NULL then).  Any of its three
 * outputs may be NULL; it returns 0, or -1 for sizes the MEAN forward refuses (a split call takes at most
 * 128 * 65 535 frames: its segments are one extent of the grid; LAST and the backward have no such limit).
 * Reference: rnn_dyn/Pooling.py:30-44 (SelectLastPooling.forward), :52-65 (MeanPooling.forward). */
#define ITTS_POOL_LAST 0
#define ITTS_POOL_MEAN 1
int itts_time_pool_plan(int n_utts, int64_t t_max, int width, int* segments, int* split, int64_t* workspace_bytes);
int itts_time_pool_fwd(const float* d_x, int64_t ldx, const int64_t* d_lens, int n_utts, int64_t t_max, int width,
                       int batch_first, int mode, float* d_y, int64_t ldy, void* d_workspace, void* stream);
/* d_dx (layout and pitch as d_x above) for d_dy [n_utts, width]: EVERY position is written, zeros included, so the
 * caller needs no memset.  MEAN: dx[b, t] = dy[b] / len_b for every t < t_max; LAST: dy[b] at the selected row.
 * Reference: autograd through rnn_dyn/Pooling.py:42-44 (the index select) and :55-64 (sum and division). */
int itts_time_pool_bwd(const float* d_dy, int64_t lddy, const int64_t* d_lens, int n_utts, int64_t t_max, int width,
                       int batch_first, int mode, float* d_dx, int64_t lddx, void* stream);
/* z = eps * exp(0.5 * log_var) + mu for d_h [M, 2L] = mu | log_var (the torch.split of rnn_dyn/VAE.py:19), d_eps and
 * d_z [M, L]; L >= 1 (an L that is no multiple of 4 takes the plain loads: the second half is off the 16-byte grid).
 * Reference: rnn_dyn/VAE.py:23-27 (VanillaVAE._reparametrize). */
int itts_vae_reparam_fwd(const float* d_h, int64_t ldh, const float* d_eps, int64_t lde, float* d_z, int64_t ldz,
                         int64_t M, int L, void* stream);
/* The whole d_dh [M, 2L] in one pass from the gradients into z, mu and log_var, each [M, L] or NULL (= zero):
 *   dh[:, :L] = dz + dmu,   dh[:, L:] = 0.5 * dz * eps * exp(0.5 * log_var) + dlog_var
 * d_h and d_eps are read only when d_dz is given.
 * Reference: autograd through rnn_dyn/VAE.py:19-27. */
int itts_vae_reparam_bwd(const float* d_dz, int64_t lddz, const float* d_dmu, int64_t lddmu, const float* d_dlv,
                         int64_t lddlv, const float* d_h, int64_t ldh, const float* d_eps, int64_t lde, float* d_dh,
                         int64_t lddh, int64_t M, int L, void* stream);
/* KL divergence of N(mu, exp(log_var)) to the standard normal with one weight per row (the sequence mask and the
 * reduction, as for itts_weighted_loss):
 *   kl_r = 0.5 * sum_c (exp(lv) + mu^2 - 1 - lv),  d_loss[0] = sum_r w[r] kl_r,
 *   d_dmu = w[r] mu,  d_dlv = 0.5 w[r] (exp(lv) - 1)  (each [M, L] or NULL),  d_elem [M] = w[r] kl_r or NULL.
 * d_mu and d_lv carry their own pitches: the two halves of h go in without a copy.  Rows of weight 0 may hold
 * anything and contribute exactly 0 to the loss and to both gradients.  A row is summed by one wave in a fixed
 * order, the rows in double through d_workspace (>= itts_vae_kld_workspace_bytes(M, L)) and a second launch.
 * Reference: loss/VAEKLDLoss.py:56-58 (loss_fn) under loss/NamedLoss.py:93-131 (mask and reduction). */
int64_t itts_vae_kld_workspace_bytes(int64_t M, int L);
int itts_vae_kld(const float* d_mu, int64_t ldmu, const float* d_lv, int64_t ldlv, const float* d_w, int64_t M, int L,
                 float* d_loss, float* d_dmu, int64_t lddmu, float* d_dlv, int64_t lddlv, float* d_elem,
                 void* d_workspace, void* stream);

/* ---- classification: softmax cross-entropy and accuracy counts (csrc/xent.hip) ------------------------------
 * Row-weighted softmax cross-entropy, loss and gradient from one call.  Per row r with target t_r, m = max_c x[r,c]:
 *   lse = m + log(sum_c exp(x[r,c] - m)),   l_r = cw[t_r] * (lse - x[r,t_r]),
 *   d_loss[0] = sum_r w[r] l_r,   d_elem[r] = w[r] l_r (or NULL),
 *   d_grad[r,c] = w[r] cw[t_r] (softmax_c - [c == t_r]) (or NULL: evaluation).
 * d_cw [C] are the class weights (NULL: ones), d_w [N] the row weights: the sequence mask and the reduction, as
 * for itts_weighted_loss and itts_vae_kld.  A row whose target is ignore_index has loss 0 and gradient 0.  A target
 * outside [0, C) that is not ignore_index is never used as an index: the row's loss is NaN (d_loss too) and its
 * gradient row zeros.  Rows of weight 0 may hold anything (bad targets, non-finite logits): they are not read and
 * contribute exactly 0.  A row's results depend on the row alone -- the same bits for any N, any row index and either
 * load form (16-byte loads when pitches are multiples of 4 floats and bases 16-byte aligned); the row losses are
 * added in double through d_workspace in one fixed order by a second launch: repeated calls give identical bits.
 * C is 1 .. 4096; everything else is refused (ITTS_E_INVALID, the message names the value) before any device work;
 * N == 0 (B == 0) succeeds and writes loss 0.
 *
 * itts_softmax_xent: class-contiguous rows d_x [N, C] with pitch ld >= C, int64 targets [N], d_grad with pitch ldg.
 * A row is shared by 1, 2, 4 .. 64 lanes (the smallest power of two with 4 * lanes >= C), from C = 257 on in
 * 2, 4, 8 or 16 steps of 256 columns; itts_xent_plan reports (lanes, steps) without device work, for the strided
 * layout (4, ceil(C / 4)): the waves that share a frame and the classes of each (kept in registers up to 64); it returns -1 for what the entry points refuse; either output may be NULL.
 * Reference: torch.nn.CrossEntropyLoss(reduction='none') under loss/NamedLoss.py:77-104 (squeeze_inputs, mask) and
 * :113-131 (_reduce).
 *
 * itts_softmax_xent_strided: class-strided d_x [B, C, T] contiguous (class c of frame (b, t) at b*C*T + c*T + t),
 * lanes along t, a frame's classes shared by the four waves of a workgroup.  The target of frame t is the arg-max over c of d_onehot (same layout) at frame t + shift, the
 * lowest index among equal maxima; the loss has T - shift frames per batch entry: d_w and d_elem are
 * [B, T - shift], d_grad is [B, C, T] and every element of it is written (zeros for t >= T - shift).
 * 0 <= shift < T.  d_workspace >= itts_softmax_xent_strided_workspace_bytes(B, T).
 * Reference: loss/OneHotCrossEntropyLoss.py:16-30.
 *
 * itts_class_counts: per row of d_x [N, C] (pitch ld) the arg-max over the classes with torch.argmax's order (the
 * lowest index among equal maxima, the first NaN if there is one).  Each output may be NULL: d_pred [N] int64;
 * d_correct[0] += rows with pred == target; d_conf [C, C] int64, [target, pred] += 1 -- both ADD to what is
 * there, so an epoch sums its batches (integer atomics: the order cannot change the sums).  Rows whose target lies
 * outside [0, C) are counted nowhere.  d_conf takes at most 1024 classes.
 * Reference: loss/UnWeightedAccuracy.py:20-35, model_trainers/ClassificationTrainer.py:34-59. */
#define ITTS_XENT_ROWS 0
#define ITTS_XENT_STRIDED 1
int itts_xent_plan(int64_t N, int C, int layout, int* lanes, int* steps);
int64_t itts_softmax_xent_workspace_bytes(int64_t N, int C);
int itts_softmax_xent(const float* d_x, int64_t ld, const int64_t* d_target, const float* d_cw, const float* d_w,
                      int64_t N, int C, int64_t ignore_index, float* d_loss, float* d_elem, float* d_grad,
                      int64_t ldg, void* d_workspace, void* stream);
int64_t itts_softmax_xent_strided_workspace_bytes(int B, int64_t T);
int itts_softmax_xent_strided(const float* d_x, const float* d_onehot, const float* d_cw, const float* d_w, int B,
                              int C, int64_t T, int shift, int64_t ignore_index, float* d_loss, float* d_elem,
                              float* d_grad, void* d_workspace, void* stream);
int itts_class_counts(const float* d_x, int64_t ld, const int64_t* d_target, int64_t N, int C, int64_t* d_pred,
                      int64_t* d_correct, int64_t* d_conf, void* stream);

/* ---- masked MSE, reduction 'mean_per_frame' (loss/NamedLoss.py:70-117) -------------------- */
/*
 * loss = mean_d( sum_{valid frames} (pred-target)^2 / n_valid ), grad = dloss/dpred.
 * d_row_valid [M] u8 (1 = frame inside the sequence, i.e. the seq mask), n_valid = number of
 * valid frames of the GLOBAL batch (sum of lengths over all ranks when data parallel).
 * d_loss: one f32 (sum over this rank's rows already divided by n_valid*D).
 * d_grad may be NULL (evaluation).  d_workspace >= itts_masked_mse_workspace_bytes(M,D).
 */
int64_t itts_masked_mse_workspace_bytes(int64_t M, int D);
int itts_masked_mse(const float* d_pred, int64_t ldp, const float* d_target, int64_t ldt,
                    const uint8_t* d_row_valid, int64_t M, int D, double n_valid,
                    float loss_weight, float* d_loss, float* d_grad, int64_t ldg,
                    void* d_workspace, void* stream);

/* The other NamedLoss types and reductions (loss/NamedLoss.py:113-131): row-weighted elementwise loss
 *   loss = sum_r w[r] sum_c e(pred[r,c] - target[r,c]),  e = squared (kind 0: MSELoss) or absolute
 *   (kind 1: L1Loss) error;  d_grad = dloss/dpred;  d_elem (optional) = w[r] e per element.
 * The sequence mask and the reduction are folded into d_row_weight [M] f32 by the caller:
 * 'mean_per_frame' mask / (frames * D), 'mean_per_sample' mask / (len_b * B * D), 'mean' mask /
 * (rows * D), 'sum' and 'none' mask.  Rows of weight 0 may hold anything.
 * d_workspace >= itts_masked_mse_workspace_bytes(M, D). */
int itts_weighted_loss(const float* d_pred, int64_t ldp, const float* d_target, int64_t ldt,
                       const float* d_row_weight, int64_t M, int D, int kind, float* d_loss,
                       float* d_grad, int64_t ldg, float* d_elem, int64_t lde, void* d_workspace,
                       void* stream);

/* ---- Adam on a flat fp32 parameter buffer (torch.optim.Adam semantics, ----------------------
 *      ModularModelHandlerPyTorch.py:570-571); grad_scale multiplies the gradient first
 *      (1/world_size after an all-reduce(sum)). */
int itts_adam_step(float* d_param, const float* d_grad, float* d_exp_avg, float* d_exp_avg_sq,
                   int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                   int64_t step, float grad_scale, void* stream);

/* Gradient norm of a flat fp32 buffer for clipping (torch.nn.utils.clip_grad_norm_,
 * ModularModelHandlerPyTorch.py:810-814): norm_kind 2 -> d_accum[0] (+)= sum x^2, norm_kind 0 ->
 * d_accum[0] = max(d_accum[0], max |x|) (infinity norm).  accumulate = 0 overwrites d_accum.
 * Deterministic two-stage reduction; d_workspace >= 4096 bytes. */
int itts_grad_norm_accum(const float* d_x, int64_t n, int norm_kind, float* d_accum,
                         int accumulate, void* d_workspace, void* stream);

/* The whole optimiser tail of one training step in one pass over a flat parameter buffer
 * (ModularModelHandlerPyTorch.py:810-831 + ExponentialMovingAverage.py:32-45):
 *   g = grad * grad_scale
 *   d_norm_accum != NULL: g *= min(1, clip_max_norm / (norm + 1e-6)), norm = sqrt(accum) (kind 2)
 *                         or accum (kind 0) of the scaled gradient    [clip_grad_norm_]
 *   clip_value > 0:       g = clamp(g, -clip_value, clip_value)        [clip_grad_value_]
 *   Adam update as itts_adam_step
 *   d_ema_shadow != NULL: shadow -= (1 - ema_decay) * (shadow - param_new) */
int itts_adam_step_fused(float* d_param, const float* d_grad, float* d_exp_avg,
                         float* d_exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                         float eps, float weight_decay, int64_t step, float grad_scale,
                         const float* d_norm_accum, int norm_kind, float clip_max_norm,
                         float clip_value, float* d_ema_shadow, float ema_decay, void* stream);

/* SGD on a flat fp32 buffer (torch.optim.SGD semantics, ModularModelHandlerPyTorch.py:572-573):
 * g += weight_decay*p; with momentum: buf = g on the first step, else momentum*buf +
 * (1-dampening)*g; g = nesterov ? g + momentum*buf : buf; p -= lr*g.  d_momentum_buf may be NULL
 * when momentum == 0. */
int itts_sgd_step(float* d_param, const float* d_grad, float* d_momentum_buf, int64_t n, float lr,
                  float momentum, float dampening, float weight_decay, int nesterov,
                  int first_step, float grad_scale, void* stream);

/* Exponential moving average of the parameters, shadow -= (1-decay)*(shadow - param)
 * (neural_networks/pytorch/ExponentialMovingAverage.py:32-45). */
int itts_ema_update(float* d_shadow, const float* d_param, int64_t n, float decay, void* stream);

/* ---- WORLD analysis, frame-parallel part --------------------------------------------------------
 * Utterances are stored back to back: d_x holds the (pre-emphasised) f64 waveforms, h_x_off[U+1]
 * their sample offsets, h_f_off[U+1] the frame offsets with
 * frames(u) = int(1000*n_u/fs/frame_period)+1 and frame i at time i*frame_period/1000 s
 * (pyworld.wav2world, src/data_preparation/world/WorldFeatLabelGen.py:792-793). */

/* CheapTrick spectral envelope (WORLD cheaptrick.cpp; q1 = -0.15, f0 floor 71 Hz in wav2world)
 * with SPTK mel-cepstral analysis optionally fused behind it, i.e.
 *   sp   = pyworld.cheaptrick(x, f0, t, fs, fft_size=fft_size)            -> d_sp [Ttot, K] f64 power
 *   mcep = pysptk.mcep(sqrt(sp), order, alpha, eps, min_det=0, etype=1, itype=3)
 *          (AudioProcessing.extract_mcep, src/data_preparation/audio/AudioProcessing.py:142-153)
 * d_sp may be NULL when only mcep is wanted (the envelope then never leaves the chip).
 * d_mc_f32 [Ttot, ld_mc] and/or d_mc_f64 [Ttot, order+1]; d_iters [Ttot] Newton steps (optional). */
int itts_cheaptrick_mcep(const double* d_x, const int64_t* h_x_off, const double* d_f0,
                         const int64_t* h_f_off, int n_utts, int fs, double frame_period_ms,
                         int fft_size, double q1, double* d_sp, int order, double alpha, double eps,
                         int miniter, int maxiter, double threshold, float* d_mc_f32, int64_t ld_mc,
                         double* d_mc_f64, int* d_iters, void* stream);

/* pysptk.mcep on a given amplitude spectrum d_amp_sp [T, K] f64 (AudioProcessing.py:146-152). */
int itts_mcep(const double* d_amp_sp, int64_t T, int K, int order, double alpha, double eps,
              int miniter, int maxiter, double threshold, float* d_mc_f32, int64_t ld_mc,
              double* d_mc_f64, int* d_iters, void* stream);

/* pysptk.mgc2sp(mc, alpha, gamma=0, fftlen): d_logamp_f64 [T, fftlen/2+1] = real part (log
 * amplitude); d_amp_f32 = exp(float32(real)) as AudioProcessing.mcep_to_amp_sp (:252-256);
 * d_pow_f64 = float64(d_amp_f32)^2, the power spectrum world_features_to_raw hands to WORLD
 * (WorldFeatLabelGen.py:925). Any of the three outputs may be NULL. */
int itts_mgc2sp(const double* d_mc, int64_t T, int order, double alpha, int fftlen,
                float* d_amp_f32, double* d_logamp_f64, double* d_pow_f64, void* stream);

/* pysptk.mgcep(amp_sp, order, alpha, gamma, eps, min_det=0, etype=1, itype=3) with pysptk's defaults
 * num_recursions = K - 1, otype = 0 (AudioProcessing.extract_mgc, AudioProcessing.py:123-140; the
 * reference uses gamma = -1/3): d_amp_sp [T, K] f64 amplitude spectra (input_is_power != 0: power
 * spectra, e.g. CheapTrick's output) -> mel-generalized cepstra d_mgc_f32 [T, ld_mgc] and / or
 * d_mgc_f64 [T, order+1]; d_iters [T] Newton steps after the initial gamma = -1 step (optional).
 * -1 <= gamma <= 0, order <= 63. */
int itts_mgcep(const double* d_amp_sp, int input_is_power, int64_t T, int K, int order, double alpha,
               double gamma, double eps, int miniter, int maxiter, double threshold,
               float* d_mgc_f32, int64_t ld_mgc, double* d_mgc_f64, int* d_iters, void* stream);
/* pysptk.mgc2sp(mgc, alpha, gamma, fftlen) (AudioProcessing.mgc_to_amp_sp, AudioProcessing.py:259-275):
 * outputs as itts_mgc2sp; gamma = 0 is itts_mgc2sp. */
int itts_mgc2sp_gamma(const double* d_mgc, int64_t T, int order, double alpha, double gamma,
                      int fftlen, float* d_amp_f32, double* d_logamp_f64, double* d_pow_f64,
                      void* stream);

/* pyworld.code_aperiodicity (WorldFeatLabelGen.py:805) / pyworld.decode_aperiodicity (:940-941). */
int itts_code_aperiodicity(const double* d_ap, int64_t T, int fft_size, int fs, double* d_bap_f64,
                           float* d_bap_f32, void* stream);
int itts_decode_aperiodicity(const double* d_bap, int64_t T, int fs, int fft_size, double* d_ap,
                             void* stream);
/* The same for the synthesis that follows (WorldFeatLabelGen.py:940-945): only the rows a voiced pulse can read --
 * frames with f0 > 0 and their two neighbours, d_f0 [T] f64 -- are written; the rest of d_ap is left untouched. */
int itts_decode_aperiodicity_voiced(const double* d_bap, const double* d_f0, int64_t T, int fs,
                                    int fft_size, double* d_ap, void* stream);

/* StoneMask F0 refinement (pyworld.stonemask; second stage of wav2world; also
 * src/data_preparation/world/LF0LabelGen.py:263-264). d_f0_in / d_f0_out [Ttot] f64. */
int itts_stonemask(const double* d_x, const int64_t* h_x_off, const double* d_f0_in,
                   const int64_t* h_f_off, int n_utts, int fs, double frame_period_ms,
                   double* d_f0_out, void* stream);

/* D4C band aperiodicity with LoveTrain V/UV (pyworld.d4c, threshold 0.85 in wav2world).
 * d_ap [Ttot, fft_size/2+1] f64 (may be NULL) and / or the coded band aperiodicity
 * pyworld.code_aperiodicity(ap, fs) as f64 [Ttot, nap] / f32 [Ttot, ld_bap] (may be NULL). */
int itts_d4c(const double* d_x, const int64_t* h_x_off, const double* d_f0, const int64_t* h_f_off,
             int n_utts, int fs, double frame_period_ms, int fft_size, double threshold,
             double* d_ap, double* d_bap_f64, float* d_bap_f32, int64_t ld_bap, void* stream);

/* DIO F0 estimation (pyworld.dio defaults: f0_floor 71, f0_ceil 800, channels_in_octave 2,
 * speed 1, allowed_range 0.1; first stage of wav2world, WorldFeatLabelGen.py:792-793).
 * d_f0 [Ttot] f64. Scratch is taken from the stream-ordered allocator (hipMallocAsync). */
int itts_dio(const double* d_x, const int64_t* h_x_off, const int64_t* h_f_off, int n_utts, int fs,
             double frame_period_ms, double f0_floor, double f0_ceil, double channels_in_octave,
             double allowed_range, double* d_f0, void* stream);

/* Harvest F0 estimation (pyworld.harvest(x, fs, f0_floor=71, f0_ceil=800, frame_period=5): the
 * estimator BASELINE.json's north_star names beside DIO; the reference's own extractor is
 * dio + stonemask, WorldFeatLabelGen.py:792-793).  Frame count per utterance:
 * itts_harvest_num_frames (WORLD GetSamplesForHarvest).  d_f0 [Ttot] f64.  The d_dbg_* pointers
 * (NULL, or device buffers when n_utts == 1) receive intermediate stages on the 1 ms grid
 * T1 = itts_harvest_num_frames(n, fs, 1.0): raw band candidates [channels, T1]; refined candidates
 * and scores after RemoveUnreliableCandidates [T1, max_candidates]; the contour before smoothing
 * [T1].  Synchronises the stream once at the end (event-list overflow check). */
int64_t itts_harvest_num_frames(int64_t n_samples, int fs, double frame_period_ms);
int itts_harvest(const double* d_x, const int64_t* h_x_off, const int64_t* h_f_off, int n_utts,
                 int fs, double frame_period_ms, double f0_floor, double f0_ceil, double* d_f0,
                 double* d_dbg_raw, double* d_dbg_cand, double* d_dbg_score, double* d_dbg_best,
                 void* stream);

/* pyworld.wav2world(x, fs, fft_size=..., frame_period=...) in one call (WorldFeatLabelGen.py:792-793):
 * DIO -> StoneMask -> CheapTrick -> D4C with wav2world's defaults (f0 floor 71 Hz, q1 -0.15, D4C
 * threshold 0.85).  d_f0 [Ttot] f64, d_sp / d_ap [Ttot, fft_size/2+1] f64 (either may be NULL);
 * fft_size <= 0: pyworld.get_cheaptrick_fft_size(fs). */
int itts_wav2world(const double* d_x, const int64_t* h_x_off, const int64_t* h_f_off, int n_utts,
                   int fs, double frame_period_ms, int fft_size, double* d_f0, double* d_sp,
                   double* d_ap, void* stream);

/* WORLD synthesis (pyworld.synthesize(f0, sp, ap, fs, frame_period)) followed by the reference's
 * float32 cast and de-pre-emphasis lfilter([1],[1,-preemphasis]) -- WorldFeatLabelGen.py:943-945.
 * d_f0 [Ttot] f64, d_sp / d_ap [Ttot, fft_size/2+1] f64 (power spectrum / aperiodicity);
 * h_y_off[U+1] sample offsets with y_len(u) = int(T_u*frame_period*fs/1000).
 * d_y_f32 and / or d_y_f64 [Ytot] (f64 = what scipy.signal.lfilter returns). */
int itts_world_synthesize(const double* d_f0, const double* d_sp, const double* d_ap,
                          const int64_t* h_f_off, const int64_t* h_y_off, int n_utts, int fs,
                          double frame_period_ms, int fft_size, double preemphasis, float* d_y_f32,
                          double* d_y_f64, void* stream);
/* The same, with the spectra still being produced when the call is made: everything in front of the pulse kernels (the
 * per-sample phase, the pulse positions, the noise: a third of the launches, bound by latency) needs d_f0 only.  `stream`
 * waits for `envelope_ready_event` (a hipEvent_t recorded behind the producer of d_sp on whatever stream it ran) right
 * before the kernel of the unvoiced pulses, which read the envelope only, and for `aperiodicity_ready_event` (behind
 * the producer of d_ap) before the kernel of the voiced ones.  NULL: that array is complete on `stream`. */
int itts_world_synthesize_after(const double* d_f0, const double* d_sp, const double* d_ap,
                                const int64_t* h_f_off, const int64_t* h_y_off, int n_utts, int fs,
                                double frame_period_ms, int fft_size, double preemphasis,
                                float* d_y_f32, double* d_y_f64, void* stream, void* envelope_ready_event,
                                void* aperiodicity_ready_event);

/* ---- acoustic model: (Bi)LSTM recurrence (torch.nn.LSTM inside rnn_dyn/RNNWrapper.py:45-107) ------
 * Packed rows, the layout pack_padded_sequence produces (RNNWrapper.py:89-92): the B sequences are
 * sorted by decreasing length, frame t of sequence b is packed row d_row_off[t] + b with
 * d_row_off[t] = sum_{t' < t} #{b : len_b > t'}; N = sum of the lengths rows in total, T = the
 * longest length.  Direction d owns column block d of every tensor.
 *   d_gin    [N, ndir*4H]    x W_ih^T + b_ih + b_hh for all frames (one itts_linear_fwd call)
 *   d_whh    [ndir][4H][H]   gate order i, f, g, o
 *   d_h0/c0  [ndir][H] or NULL (zeros)
 *   d_lengths [B] int32 on the device, h_lengths the same values on the host (sorted decreasingly;
 *            the host copy sizes the per-step launches), d_row_off [T] int32 on the device;
 *   d_rev_row [T*B] int32 on the device (needed when ndir == 2): the reverse direction starts at
 *            each sequence's own last frame, at step s it visits packed row
 *            d_rev_row[s*B + b] = d_row_off[len_b - 1 - s] + b (entries with s >= len_b unused)
 *   d_y      [N, ndir*H]
 *   d_gates [N, ndir, H, 4] (i, f, g, o after activation, gate-minor) and d_csave [N, ndir*H] (c_t):
 *            saved for the backward pass, both NULL for inference.  h_{t-1}, which dW_hh needs next
 *            to d_dg, is d_y shifted by one frame along each sequence (h0 at the first frame).
 *   d_hn/d_cn [ndir][B][H]   final states in sorted row order (may be NULL);
 *   d_state >= itts_lstm_state_bytes bytes */
int64_t itts_lstm_state_bytes(int B, int H, int ndir);
int itts_lstm_layer_fwd(const float* d_gin, const float* d_whh, const float* d_h0, const float* d_c0,
                        const int* d_lengths, const int* h_lengths, const int* d_row_off,
                        const int* d_rev_row, int T, int B, int H, int ndir, float* d_y,
                        float* d_gates, float* d_csave, float* d_hn, float* d_cn, void* d_state,
                        void* stream);
/* d_dg [N, ndir*4H] = dLoss/d(pre-activation gates) from d_dy [N, ndir*H]; d_whh as in the
 * forward call.  dW_ih, dW_hh, db and dX follow from d_dg with itts_linear_bwd_weight /
 * itts_linear_bwd_input.  d_dc0 [ndir][B][H] (may be NULL) receives dLoss/d(initial cell state) per
 * packed row (RNNWrapper's train_hidden_init, rnn_dyn/RNNWrapper.py:66-71: sum over the rows);
 * dLoss/d(initial hidden state) of row b is W_hh^T d_dg[first processed frame of b]. */
int itts_lstm_layer_bwd(const float* d_dy, const float* d_whh, const float* d_c0,
                        const float* d_gates, const float* d_csave, const int* h_lengths,
                        const int* d_row_off, const int* d_rev_row, int T, int B, int H, int ndir,
                        float* d_dg, float* d_dc0, void* d_state, void* stream);

/* ---- (Bi)GRU recurrence (torch.nn.GRU behind rnn_dyn/RNNWrapper.py:45-107 for `..GRU..` groups;
 *      gate order r, z, n; packed rows, lengths and row offsets as for the LSTM entry points).
 * d_gin  [N, ndir*3H] = X W_ih^T + b_ih for all frames (one itts_linear_fwd call),
 * d_whh  [ndir][3H][H], d_bhh [ndir][3H] (b_hn sits inside r * (W_hn h + b_hn)), d_h0 [ndir][H] or
 * NULL.  Training saves d_gates [N, ndir, H, 4] = (r, z, n after activation, W_hn h + b_hn) per
 * unit; NULL for inference.  d_hn [ndir][B][H] may be NULL.
 * d_state >= itts_gru_state_bytes(B, H, ndir).
 * Backward takes d_hprev [N, ndir*H] (h_{t-1} of every frame: d_y shifted by one frame along each
 * sequence, h0 at the first frame) and fills d_dgi (gradient wrt d_gin: feeds dX, dW_ih, db_ih) and d_dgh (gradient wrt the
 * hidden projections: feeds dW_hh with d_hprev, db_hh), both [N, ndir*3H].  d_dh0 [ndir][B][H] (may
 * be NULL) receives the direct part dh * z of dLoss/d(initial hidden state) per packed row; the
 * recurrent part of row b is W_hh^T d_dgh[first processed frame of b] (train_hidden_init). */
int64_t itts_gru_state_bytes(int B, int H, int ndir);
int itts_gru_layer_fwd(const float* d_gin, const float* d_whh, const float* d_bhh,
                       const float* d_h0, const int* d_lengths, const int* h_lengths,
                       const int* d_row_off, const int* d_rev_row, int T, int B, int H, int ndir,
                       float* d_y, float* d_gates, float* d_hn, void* d_state, void* stream);
int itts_gru_layer_bwd(const float* d_dy, const float* d_whh, const float* d_gates,
                       const float* d_hprev, const int* h_lengths,
                       const int* d_row_off, const int* d_rev_row, int T, int B, int H, int ndir,
                       float* d_dgi, float* d_dgh, float* d_dh0, void* d_state, void* stream);

/* ---- vanilla (Bi)RNN recurrence (torch.nn.RNN behind rnn_dyn/RNNWrapper.py:45-107 for `..RNNTANH..` / `..RNNRELU..`
 *      groups): h_t = act(gin_t + W_hh h_{t-1}), act = ITTS_ACT_TANH or ITTS_ACT_RELU; packed rows, lengths, row
 *      offsets and the reverse row table as for the LSTM entry points.
 * d_gin [N, ndir*H] = X W_ih^T + b_ih + b_hh for all frames (one itts_linear_fwd call), d_whh [ndir][H][H], d_h0
 * [ndir][H] or NULL (zeros), d_y [N, ndir*H], d_hn [ndir][B][H] in sorted row order (may be NULL; row b's is d_y at
 * the last frame its direction processes).  H is a multiple of 16 (run other sizes zero-padded).  Nothing but d_y is
 * saved for backward, so a training and an inference call are the same call.
 * d_state >= itts_rnn_layer_state_bytes(B, H, ndir) = 4 * (4 * ndir * B * H + ndir * H * H) bytes: the running state
 * and the carried gradient, two step parities each, and the re-tiled W_hh; 0 for a size that is not positive.
 * Backward takes d_y and fills d_dg [N, ndir*H] = (d_dy + d_dg[next processed frame] W_hh) * act'(d_y), act' = 1 - y^2
 * or y > 0, the gradient wrt d_gin and wrt the hidden projection alike: dX, dW_ih and both bias gradients follow from
 * it as for the LSTM, dW_hh from it and d_y shifted by one frame along each sequence (h0 at the first frame);
 * dLoss/d(initial hidden state) of row b is W_hh^T d_dg[first processed frame of b].  A gradient into d_hn is added to
 * d_dy at the row's last processed frame before the call.
 * Bad arguments (H % 16, another activation code, a null operand, lengths that are not sorted / T not the longest)
 * return ITTS_E_INVALID before any device work.  These layers always run on the per-step kernels. */
int64_t itts_rnn_layer_state_bytes(int B, int H, int ndir);
int itts_rnn_layer_fwd(const float* d_gin, const float* d_whh, const float* d_h0, const int* d_lengths,
                       const int* h_lengths, const int* d_row_off, const int* d_rev_row, int T, int B, int H,
                       int ndir, int act /* ITTS_ACT_TANH | ITTS_ACT_RELU */, float* d_y, float* d_hn,
                       void* d_state, void* stream);
int itts_rnn_layer_bwd(const float* d_dy, const float* d_whh, const float* d_y, const int* h_lengths,
                       const int* d_row_off, const int* d_rev_row, int T, int B, int H, int ndir, int act,
                       float* d_dg, void* d_state, void* stream);
/* out = forward, backward vanilla RNN layer calls of this process that passed their argument checks (process-wide
 * atomic counts, no device call).  itts_rnn_path_counts below does not count them. */
int itts_rnn_layer_counts(int64_t out[2]);

/* Which kernel the dense-layer products (itts_linear_*) of this process ran on (process-wide atomic counts, no device
 * call): out[e] = products on the LDS-DMA ring kernel, out[4 + e] = on the register-staged kernel, e = the epilogue
 * kind: 0 plain store (weight gradients, input gradients without an activation), 1 bias + activation (forward),
 * 2 activation derivative (input gradients), 3 masked MSE (itts_linear_fwd_mse).  The two products of a fused
 * itts_linear_bwd launch count one each. */
int itts_gemm_path_counts(int64_t out[8]);
/* What the last dense call of the calling host thread launched (itts_linear_fwd, itts_linear_fwd_mse,
 * itts_linear_bwd_input, itts_linear_bwd_weight, itts_linear_bwd; thread-local, no device call).  Each of them clears
 * the record on entry, each of its launches appends one entry of 16 int32, written at the launch site from the template
 * parameters and arguments of that launch.  Returns the number of launches; the first min(that, max_entries, 8) entries
 * go to out (may be NULL), in launch order:
 *   a product      {kernel (1 register-staged, 2 ring, 3 ring pair launch), A_ROW, B_ROW, epilogue (as above), TN,
 *                   STAGES (staged; 0 otherwise), WM (ring: 1 = 64 x 128 tiles, 2 = 128 x 64; 0 otherwise), vecA, vecB,
 *                   the wide-store epilogue is the one taken, grouped tile order, split-K slabs, activation family
 *                   (0 none / Tanh / ReLU, 1 the others), tiles, workgroups, 1 where the
 *                   epilogue applied dropout (the _dropout entry points) and 0 otherwise}; a pair launch gives two
 *                   entries, the weight-gradient product first
 *   a reduction    {4, float4 (1) or scalar (0) columns, merged with the bias, deferred (itts_defer_reductions),
 *                   slabs, 0 ...} */
int itts_gemm_last_plan(int32_t* out, int max_entries);

/* Which way the LSTM / GRU layer calls of this process went (process-wide atomic counts, no device call):
 * out = forward ran, declined, gave_up, backward ran, declined, gave_up.  `ran`: the persistent recurrence did
 * the layer; `declined`: it was not launched (ITTS_RNN_PERSISTENT=0, H != 512, device not ready, cooling down)
 * and the per-step kernels did the layer; `gave_up`: a launch failed or came back with its abort flag set, and
 * the per-step kernels redid the layer. */
int itts_rnn_path_counts(int64_t out[6]);

/* ---- corpus audio preparation (csrc/audio_prep.hip): the four steps that scripts/bash_utils.sh runs over the wav
 *      corpus before gen_data -- src/data_preparation/audio/down_sampling.py, silence_remove.py,
 *      normalize_loudness.py, high_pass_filter.py.  float64 throughout; the signals of a batch lie back to back in
 *      d_x, signal s = d_x[h_offsets[s] .. h_offsets[s + 1]), h_offsets [n_signals + 1] ascending from 0.  Every sum
 *      runs in a fixed order that depends on the signal alone: a signal's result has the same bits alone and at any
 *      place of any batch.  Bad arguments (a null pointer, the cases named below) return ITTS_E_INVALID with a message
 *      naming the value before any device work -- a size that would need more than 2^24 - 1 workgroups in one launch
 *      (16 M signals, 16 M frames of one signal, a signal of 3e10 samples) among them; n_signals == 0 succeeds and does
 *      nothing.
 *
 * itts_fir_filtfilt_batch: scipy.signal.filtfilt(b, [1], x) (high_pass_filter.py:57; padtype "odd", padlen =
 *   3 * numtaps) with the numtaps coefficients d_taps, into d_y (same offsets).  numtaps is odd, 1 .. 2047; every
 *   signal is longer than padlen.  d_workspace >= itts_fir_filtfilt_workspace_bytes(h_offsets[n_signals], n_signals,
 *   numtaps) bytes (the first pass: n + padlen values per signal; 0 for sizes that are not positive).
 * itts_resample_poly_batch: scipy.signal.resample_poly(x, up, down) (the librosa.load(sr=...) of
 *   down_sampling.py:43, on scipy's polyphase resampler) with the filter d_taps designed by the caller --
 *   firwin(2 * half + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up, half = 10 * max(up, down), for scipy's
 *   defaults; numtaps odd, its centre tap aligned with the first sample -- zeros outside the signal.  up and down are
 *   1 .. 1024 (reduce them by their gcd first).  Signal s fills d_y[h_out_offsets[s] .. h_out_offsets[s + 1]), which
 *   has to be ceil(n * up / down) long.
 * itts_loudness_normalise_batch: y = (x - mean(x)) * sqrt(n * ref_rms^2 / sum((x - mean(x))^2))
 *   (normalize_loudness.py:41-42), ref_rms > 0; d_y may be d_x.  A constant signal gives non-finite values, as there.
 * itts_frame_rms_batch: librosa.feature.rms(y=x, frame_length, hop_length=hop, center=True)
 *   (librosa.effects.trim behind silence_remove.py:75-79): the signal padded by frame_length / 2 on both sides --
 *   ITTS_PAD_CONSTANT with zeros (librosa >= 0.10), ITTS_PAD_REFLECT mirrored (librosa 0.8 / 0.9) -- and one
 *   sqrt(mean square) per frame into d_rms[h_frame_offsets[s] ..]; signal s has
 *   1 + (n + 2 * (frame_length / 2) - frame_length) / hop frames (1 + n / hop for an even frame_length) and is not
 *   empty; hop >= 1. */
#define ITTS_PAD_CONSTANT 0
#define ITTS_PAD_REFLECT 1
int64_t itts_fir_filtfilt_workspace_bytes(int64_t n_total, int n_signals, int numtaps);
int itts_fir_filtfilt_batch(const double* d_x, const int64_t* h_offsets, int n_signals, const double* d_taps,
                            int numtaps, double* d_y, void* d_workspace, void* stream);
int itts_resample_poly_batch(const double* d_x, const int64_t* h_offsets, const int64_t* h_out_offsets,
                             int n_signals, int up, int down, const double* d_taps, int numtaps, double* d_y,
                             void* stream);
int itts_loudness_normalise_batch(const double* d_x, const int64_t* h_offsets, int n_signals, double ref_rms,
                                  double* d_y, void* stream);
int itts_frame_rms_batch(const double* d_x, const int64_t* h_offsets, const int64_t* h_frame_offsets, int n_signals,
                         int frame_length, int hop, int pad_mode, double* d_rms, void* stream);

/* ---- raw-waveform targets (csrc/mol.hip): the discretized mixture-of-logistics loss of a 16-bit sample-level
 *      vocoder, the mu-law reader behind the one-hot loss, and the linear up-sampling of conditioning features.
 *
 * itts_mol_loss: loss/DiscretizedMixturelogisticLoss.py:23-136, loss and gradient from one launch.  d_x [B, 3K, T]
 * contiguous float32 (channels 0 .. K mixture logits, K .. 2K means, 2K .. 3K log-scales), d_y [B, 1, T] targets in
 * [-1, 1]; lanes run along t; frame t of the input is scored against y[t + shift], so the loss has T - shift frames
 * per batch entry: d_w (row weights: mask and reduction) and d_elem (w l, or NULL) are [B, T - shift], d_grad (or NULL)
 * is [B, 3K, T] and every element of it is written (zeros for t >= T - shift and for rows of weight 0).  Per frame and
 * mixture, with s = max(log-scale, log_scale_min), h = 1 / (num_classes - 1), u = e^-s (y - mean + h),
 * v = e^-s (y - mean - h), m = e^-s (y - mean):
 *   y < -0.999: log sigmoid(u);   y > 0.999: log(1 - sigmoid(v));   else with
 *   delta = sigmoid(u) - sigmoid(v) = sigmoid(u) sigmoid(-v) (1 - e^-(2 h e^-s)) (no cancellation):
 *   delta > 1e-5: log delta;   else m - s - 2 softplus(m) - log((num_classes - 1) / 2);
 * plus log_softmax of the logits; l = -logsumexp over the K mixtures, with hinge != 0 plus
 * sum_k max(0, -log-scale_k - log(num_classes)) on the UNCLAMPED log-scales (:124-132).  The gradient is autograd's
 * of exactly this: the selected branch only, nothing through the clamp below log_scale_min,
 * softmax(logit) - responsibility on the logits, -1 from an active hinge term.  d_loss[0] = sum w l, added in double
 * through d_workspace (>= itts_mol_loss_workspace_bytes(B, T)) by a second launch in a fixed order: repeated calls
 * give identical bits; a frame's results depend on that frame alone (any B, any position); rows of weight 0 are never
 * read and contribute exactly 0.  No float atomics.  B == 0 succeeds with loss 0.  K outside 1 .. 64, num_classes < 2,
 * shift outside 0 .. T - 1 and T < 1 are refused (ITTS_E_INVALID, the message names the value) before any device work.
 *
 * The three below take a batch of signals back to back behind host offsets, as the audio preparation does; a
 * signal's values do not depend on its place in the batch; n_signals == 0 succeeds and does nothing.
 * itts_mulaw_encode_f64: RawWaveformLabelGen.py:164-167, float64 in, int64 index out:
 *   trunc((sign(x) log(1 + mu |x|) / log(1 + mu) + 1) mu / 2), mu 1 .. 65535.
 * itts_mulaw_decode: :169-173, int64 index in, float64 out: r = i / (mu / 2) - 1, sign(r) / mu ((1 + mu)^|r| - 1).
 * itts_mulaw_onehot: the [n, mu + 1] float32 one-hot targets of :92-94 from the float64 signals in one launch;
 *   signal s reads d_x[h_begin[s] ..] (after the silence trim) and fills the rows h_out_offsets[s] ..
 *   h_out_offsets[s + 1] of d_onehot, every element of them written.
 * itts_sample_linearly: misc/utils.py:89-100, [T, D] rows to [m T, D] at linspace(0, T - 1, m T), interpolated as
 *   scipy's interp1d does it -- the slope y_hi - y_lo in the input's precision, slope (x - lo) + y_lo in float64 --
 *   and stored as float32 (out_f64 == 0) or float64; in_f64 says which the input is.  Signal s has
 *   h_offsets[s + 1] - h_offsets[s] >= 2 rows of D values and fills the rows m h_offsets[s] .. of d_y; m >= 1, D >= 1.
 *   The first and the last output row are the input's. */
int64_t itts_mol_loss_workspace_bytes(int B, int64_t T);
int itts_mol_loss(const float* d_x, const float* d_y, const float* d_w, int B, int K, int64_t T, int shift,
                  int num_classes, double log_scale_min, int hinge, float* d_loss, float* d_elem, float* d_grad,
                  void* d_workspace, void* stream);
int itts_mulaw_encode_f64(const double* d_x, const int64_t* h_offsets, int n_signals, int mu, int64_t* d_index,
                          void* stream);
int itts_mulaw_decode(const int64_t* d_index, const int64_t* h_offsets, int n_signals, int mu, double* d_y,
                      void* stream);
int itts_mulaw_onehot(const double* d_x, const int64_t* h_begin, const int64_t* h_out_offsets, int n_signals, int mu,
                      float* d_onehot, void* stream);
int itts_sample_linearly(const void* d_x, int in_f64, const int64_t* h_offsets, int n_signals, int D, int m,
                         void* d_y, int out_f64, void* stream);

/* ---- the WaveNet vocoder network (csrc/wavenet.hip; models/WaveNetWrapper.py:110-132 wraps the external
 *      wavenet_vocoder package: the teacher-forced forward of :117 and the per-sample incremental_forward of :126).
 *
 * itts_glu_gate_fwd (WaveNetWrapper.py:110-132, the gate of a residual layer inside :117): z [N, G / 2] =
 *   tanh(a + ca) * sigmoid(b + cb) from x [N, G] = a | b and the optional c [N, G] = ca | cb (NULL: absent); row
 *   pitches in floats.  float4 rows when G / 2 and every pitch are multiples of 4 and the bases 16-byte aligned, the
 *   scalar form otherwise.  G even and >= 2.
 * itts_glu_gate_bwd (WaveNetWrapper.py:110-132): dx [N, G] from dz [N, G / 2], recomputed from the same x and c; dx
 *   is also the gradient of c.
 * itts_wavenet_state_floats (WaveNetWrapper.py:110-132): floats of the ring-buffer scratch itts_wavenet_generate needs
 *   for B rows: ceil(B / 16) * sum_l ((kernel_size - 1) * dilation_l + 1) * 16 * residual_channels; -1 (and a
 *   message) for a geometry outside the envelope below.
 * itts_wavenet_generate (WaveNetWrapper.py:110-132, the incremental_forward of :126 for whole batches): every sample
 *   of every row in one launch; one workgroup per 16 rows, no synchronisation beyond the workgroup barrier.  Weights
 *   are the EFFECTIVE ones (weight norm applied), packed by the caller: an operand W [K, N] (K, N multiples of 16,
 *   zero filled) as image[K / 16][N / 16][64][4] with image[kb][tile][lane][j] = W[16 kb + 4 (lane >> 4) + j]
 *   [16 tile + (lane & 15)].
 *     d_wf [Cin0, R], d_bf [R]: first conv, row c = the weight column of class c (Cin0 = out_channels; scalar_input:
 *       Cin0 = 1);
 *     d_w1 [layers] images of [kernel_size R + cin16, G] (rows j R + r: tap j of conv, the tap at t - (kernel_size -
 *       1 - j) dilation; rows kernel_size R + i: conv1x1c; cin16 = cin rounded up to 16), d_b1 [layers, G];
 *     d_w2 [layers] images of [G / 2, R + S] (columns: conv1x1_out | conv1x1_skip), d_b2 [layers, R + S];
 *     d_wh1 image of [S, S], d_bh1 [S]; d_wh2 image of [S, C16], d_bh2 [C16] (C16 = out_channels rounded up to 16).
 *   d_c [B, Tc, cin] conditioning at the sample rate (NULL with cin 0), d_u the uniforms ([B, T_out], scalar_input:
 *   [B, T_out, 2], in (0, 1)), h_lengths [B] host, each 0 .. T_out.  d_out [B, T_out]: int32 classes, or float
 *   samples with scalar_input (then the output is 3 K mixture-of-logistics parameters); d_logits [B, T_out,
 *   out_channels] or NULL.  Only positions t < h_lengths[b] are written.  initial_class: the class fed at step 0, -1
 *   for the all-zero input.  A row's bits do not depend on B or its position; repeated calls give identical bits.
 *   Envelope (anything else: ITTS_E_INVALID with a message, before any device work): kernel_size 2 or 3; R and S
 *   multiples of 16 up to 512; G a multiple of 32 up to 512; cin 0 .. 128; out_channels 2 .. 256, scalar_input:
 *   3 K with K <= 64; layers 1 .. 64; dilations 1 .. 512. */
int itts_glu_gate_fwd(const float* d_x, int64_t ldx, const float* d_c, int64_t ldc, float* d_z, int64_t ldz, int64_t N,
                      int G, void* stream);
int itts_glu_gate_bwd(const float* d_dz, int64_t lddz, const float* d_x, int64_t ldx, const float* d_c, int64_t ldc,
                      float* d_dx, int64_t lddx, int64_t N, int G, void* stream);
int64_t itts_wavenet_state_floats(int B, int layers, int kernel_size, int residual_channels, const int* h_dilations);
int itts_wavenet_generate(const float* d_wf, const float* d_bf, const float* d_w1, const float* d_b1,
                          const float* d_w2, const float* d_b2, const float* d_wh1, const float* d_bh1,
                          const float* d_wh2, const float* d_bh2, const int* h_dilations, int layers, int kernel_size,
                          int residual_channels, int gate_channels, int skip_channels, int cin_channels,
                          int out_channels, int scalar_input, double log_scale_min, const float* d_c, int64_t Tc,
                          const float* d_u, const int* h_lengths, int B, int64_t T_out, int initial_class,
                          float* d_state, int64_t state_floats, void* d_out, float* d_logits, void* stream);

/* ---- training batches of the vocoder from a device-resident corpus (csrc/vocoder_batch.hip; what
 *      model_trainers/WaveNetVocoderTrainer.py:99-122, :141-173 gets from two readers, max_frames and a collate).
 *
 * itts_vocoder_windows: one launch writes the targets and the conditioning of B windows of W columns.  d_x [n_x]
 *   float64 samples, the utterances back to back; d_feat [n_rows, cin] float32 conditioning frames, back to back.
 *   h_windows [B, 5] host int64, per window: the index in d_x of its first sample; its length len, 1 .. W; the first
 *   row of its utterance in d_feat; the utterance's T >= 2 frames; the place a of the first sample in the utterance,
 *   a + len <= m T.  Sample a + j pairs with row a + j of itts_sample_linearly of the WHOLE utterance (m T rows), so a
 *   window's conditioning equals the slice of the up-sampled utterance, bit for bit.  For j < len:
 *     mu >= 1: d_target [B, mu + 1, W] (class-strided, as itts_softmax_xent_strided takes it) gets a 1 at the class
 *              of itts_mulaw_encode_f64 and zeros elsewhere;  mu == 0: d_target [B, 1, W] = (float) x;
 *     d_cond [B, cin, W] = the interpolated features (NULL with cin == 0; d_feat, n_rows and the last three window
 *     fields are then not looked at).
 *   Columns j >= len are zeros.  Every element of both outputs is written; lanes run along the columns, a lane
 *   computes its class and its place among the frames once and writes its column.  A window's bits depend on its five
 *   numbers alone (not on B or its place in the batch); no atomics: repeated calls give identical bits.  B == 0
 *   succeeds and does nothing.  Envelope (anything else: ITTS_E_INVALID with a message naming the value, before any
 *   device work): mu 0 .. 4095, cin 0 .. 128, m >= 1, W >= 1, B <= 65535, every window inside d_x and d_feat. */
int itts_vocoder_windows(const double* d_x, int64_t n_x, const float* d_feat, int64_t n_rows, int cin, int m, int mu,
                         const int64_t* h_windows, int B, int64_t W, float* d_target, float* d_cond, void* stream);

/* ---- Fixed (duration-derived) attention of the encoder-decoder model (csrc/fixed_attention.hip) ------------------
 * float32; pitches (ld*) are floats from one row to the next, utterance steps (utt*) floats from one utterance to the
 * next, last extents have unit stride.  16-byte accesses where every pitch, step and base of a side (phoneme side: A
 * and Abar; channel side: enc, ctx / dctx, d_enc) allows, plain ones otherwise: the same lanes, the same bits.
 *   fwd  A [B, T, P], enc [B, P, C], n = n_frames_per_step -> Abar [B, K, P], ctx [B, K, C].  K = T / n (T % n != 0
 *        is refused), with partial_last K = ceil(T / n) and the last chunk is the mean over the rows it has.
 *        Abar[b, k, :] = (sum of the chunk's rows of A in ascending frame order) / row count;
 *        ctx[b, k, :] = sum over p ascending of Abar[b, k, p] * enc[b, p, :], terms with Abar == 0 skipped (so Inf or
 *        NaN in a row of enc that no frame attends to does not reach ctx, unlike a dense product).
 *   bwd  Abar, dctx [B, K, C] -> d_enc [B, P, C], d_enc[b, p, :] = sum over k ascending of Abar[b, k, p] * dctx[b, k, :],
 *        zeros skipped; every position is written; no atomics.  A is ground truth: it has no gradient.
 *   An utterance's results depend on its own rows only (not on B or its index); repeated calls give identical bits.
 *   Envelope: P 1 .. 2048, C 1 .. 4096, n 1 .. 64; anything else is ITTS_E_INVALID with a message before any device
 *   work.  itts_fixed_attention_plan (no device work; 0, or -1 outside the envelope): K, the forward grid and its LDS
 *   bytes, the backward grid (x, y), and whether dense tensors on 16-byte bases take the 16-byte accesses. */
int itts_fixed_attention_plan(int B, int64_t T, int P, int C, int n, int partial_last, int64_t* K, int* fwd_blocks,
                              int* fwd_lds_bytes, int* bwd_blocks_x, int* bwd_blocks_y, int* vec_p, int* vec_c);
int itts_fixed_attention_fwd(const float* d_A, int64_t ldA, int64_t uttA, const float* d_enc, int64_t ldE,
                             int64_t uttE, int B, int64_t T, int P, int C, int n, int partial_last, float* d_abar,
                             int64_t ldM, int64_t uttM, float* d_ctx, int64_t ldX, int64_t uttX, void* stream);
int itts_fixed_attention_bwd(const float* d_abar, int64_t ldM, int64_t uttM, const float* d_dctx, int64_t ldX,
                             int64_t uttX, int B, int64_t K, int P, int C, float* d_denc, int64_t ldE, int64_t uttE,
                             void* stream);

/* ---- One recurrent step on per-row states (csrc/rnn_cell.hip) -----------------------------------------------------
 * h' (and c') of one time step of an LSTM / GRU / RNN layer direction for B rows with a state each:
 *   d_gi [B, G*H] = x W_ih^T + b_ih (LSTM, RNN: + b_hh), d_gh [B, G*H] = h W_hh^T, both from itts_linear_fwd;
 *   d_b_hh [3H] for the GRU (NULL otherwise); d_h / d_c [B, H] in, d_h_out / d_c_out [B, H] out (d_c* LSTM only).
 * G = 4 / 3 / 1, torch.nn's gate order; act (RNN): ITTS_ACT_TANH or ITTS_ACT_RELU.  Any H >= 1. */
#define ITTS_CELL_LSTM 0
#define ITTS_CELL_GRU 1
#define ITTS_CELL_RNN 2
int itts_rnn_cell_step(int kind, int act, const float* d_gi, int64_t ldgi, const float* d_gh, int64_t ldgh,
                       const float* d_b_hh, const float* d_h, int64_t ldh, const float* d_c, int64_t ldc, int B, int H,
                       float* d_h_out, int64_t ldho, float* d_c_out, int64_t ldco, void* stream);

/* ---- Dynamic time warping of pairs of feature sequences (csrc/dtw.hip; the scores of Metrics.get_metrics_dtw; the
 *      reference has no counterpart) ---------------------------------------------------------------------------------
 * Pair b: x[b] [T1_b, D], y[b] [T2_b, D], float32 (is_f64 = 0) or float64 (is_f64 = 1), padded to [B, T1max, D] and
 * [B, T2max, D]; ld* are elements from one frame to the next, utt* from one pair to the next, D has unit stride.
 * Nothing behind a length (or behind D in a row) is read.  All arithmetic is float64:
 *   d(i, j) = sqrt(sum_k (x[i, k] - y[j, k])^2);  C(0, 0) = d(0, 0);
 *   C(i, j) = d(i, j) + min(C(i-1, j-1), C(i-1, j), C(i, j-1)), a predecessor outside the grid or the band = +inf;
 *   on equal values the diagonal is taken, then (i-1, j), then (i, j-1).
 * band = r >= 0 admits cell (i, j) only if |j - centre(i)| <= r, centre(i) = (2 i (T2-1) + (T1-1)) / (2 (T1-1)) in
 * integer (floor) division, i.e. round-half-up of i (T2-1) / (T1-1); with T1 == 1 the one path is the whole row and
 * every cell is admitted.  So (0, 0) and (T1-1, T2-1) are always admitted.  band < 0: no band.  A band that does not
 * connect the two (r below the jump of centre(i) from one row to the next, when T2 > T1) gives cost = +inf.
 * Outputs: d_cost [B] = C(T1-1, T2-1); d_length [B] = cells on the path, L (0 when the cost is not finite);
 *   d_path [B, path_rows, 2] int32 (or NULL: no path is written), rows (i, j) from (0, 0) to (T1-1, T2-1), rows
 *   L .. path_rows - 1 set to -1; path_rows >= T1max + T2max - 1.
 * d_work: itts_dtw_workspace_bytes(B, T1max, T2max) bytes = B T1max T2max, one byte per cell (0 diagonal, 1 (i-1, j),
 *   2 (i, j-1)); the only per-cell HBM traffic, cells outside the band are not written; -1 outside the envelope.
 * One workgroup per pair and one wave per pair for the backtrack; no workgroup waits on another, no atomics: a pair's
 * bits depend on its own rows, its lengths and the band alone, repeated calls give identical bits.  h_t1 / h_t2 are
 * host arrays (copied to the device through scope-owned scratch).
 * Envelope: B >= 1, 1 <= T1_b <= T1max <= 4096, 1 <= T2_b <= T2max <= 4096, 1 <= D <= 128; anything else is
 *   ITTS_E_INVALID with a message naming the value, before any device work.
 * itts_dtw_plan (no device work; 0, or -1 outside the envelope): the columns of a block, the rows of a pass (the tile
 *   edges of the forward kernel) and 8 x the bytes stored per cell. */
int64_t itts_dtw_workspace_bytes(int B, int T1max, int T2max);
int itts_dtw_plan(int T1, int T2, int D, int* col_block, int* rows_per_pass, int* cell_bytes_x8);
int itts_dtw_align(const void* d_x, int64_t ldx, int64_t uttx, const void* d_y, int64_t ldy, int64_t utty, int is_f64,
                   const int32_t* h_t1, const int32_t* h_t2, int B, int T1max, int T2max, int D, int band,
                   double* d_cost, int32_t* d_length, int32_t* d_path, int64_t path_rows, void* d_work,
                   int64_t work_bytes, void* stream);
/* itts_dtw_step_probe: a measuring aid (scripts/bench_dtw.py).  One workgroup runs `steps` steps of a dependency chain
 *   with nothing else in them and writes its 256 doubles to d_out: mode 0, 256 threads pass a value to their neighbour
 *   through LDS with one workgroup barrier a step; mode 1, one wave passes it by a lane shift (the forward kernel's
 *   step).  (T1 + T2 - 1) x the time of a step is what no tiling of the recurrence gets under. */
int itts_dtw_step_probe(int mode, int steps, double* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IDIAPTTS_AMD_H */
