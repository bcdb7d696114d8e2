/*
 * qpnet_hip.h -- C ABI of libqpnet_hip.so: the MI355X (gfx950) QPNet hot path.
 *
 * The reference (bigpon/QPNet) has no native boundary: its hot path is the Python module
 * src/nets/qpnet.py calling stock torch ops.  The boundary that module would bind if its
 * hot path were native is defined here; each entry point cites the
 * reference interface it replaces.  The host-side mirror of the reference's Python surface
 * (class QPNet etc.) lives in qpnet_amd/qpnet.py and calls ONLY these functions.
 *
 * Conventions
 *   - plain C types; every `d_*` pointer is a DEVICE pointer owned by the caller
 *     (e.g. torch tensors' data_ptr()); `h_*` pointers are host memory.
 *   - return 0 on success, a negative QPN_E* code otherwise; nothing throws across the ABI.
 *     qpn_last_error() returns a static, human-readable description of the last failure.
 *   - the library owns only its handle and the workspaces it allocates in it.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).
 *   - a handle is bound to the device current at qpn_create(); not thread-safe per handle.
 *   - there is NO CPU fallback: every compute entry point fails with QPN_ENODEV when no
 *     HIP device is usable.
 */
#ifndef QPNET_HIP_H
#define QPNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QPN_OK 0
#define QPN_EINVAL (-1)      /* bad argument / unsupported geometry            */
#define QPN_ENODEV (-2)      /* no usable HIP device / HIP runtime error       */
#define QPN_ENOMEM (-3)      /* workspace allocation failed                    */
#define QPN_ERANGE (-4)      /* pitch-dependent gather left its ring (ref: assert qpnet.py:294,417) */
#define QPN_ESTATE (-5)      /* call order (e.g. decode before set_weights)    */

/* Constructor kwargs of QPNet (reference src/nets/qpnet.py:174-178). */
typedef struct {
    int n_quantize, n_aux, n_resch, n_skipch;
    int dilationF_depth, dilationF_repeat;
    int dilationA_depth, dilationA_repeat;
    int kernel_size, upsampling_factor;
} qpn_config;

typedef struct qpn_handle qpn_handle;

/* library / ABI version (major*1000 + minor) */
int qpn_version(void);

/* Last error message of this thread's most recent failing call. */
const char* qpn_last_error(void);

/* Number of fp32 parameters of the geometry = length of the flat parameter vector, which is
 * the concatenation of state_dict() tensors in registration order, each in its native
 * PyTorch layout (reference QPNet.__init__, src/nets/qpnet.py:200-235). */
int64_t qpn_param_count(const qpn_config* cfg);

/* QPNet.__init__ (src/nets/qpnet.py:174-237): validate geometry, build the decode program. */
int qpn_create(const qpn_config* cfg, qpn_handle** out);
void qpn_destroy(qpn_handle* h);

/* load_state_dict / .cuda() (reference bin/qpnet_decode.py:286-293): bind the flat fp32
 * parameter vector (device memory, n == qpn_param_count) and (re)pack the decode tiles.
 * The vector is read again by every later call; call again after the values change.
 * Stream-ordered, no host synchronisation. */
int qpn_set_weights(qpn_handle* h, const float* d_flat, size_t n, void* stream);

/* mode of qpn_decode */
#define QPN_MODE_ARGMAX 0
#define QPN_MODE_SAMPLING 1

/*
 * QPNet.batch_fast_generate (reference src/nets/qpnet.py:314-559), all batch rows at once: persistent kernels that loop
 * over all samples of their utterances, launched once per call.  The launch plan is sized from the device's CU count
 * (hipDeviceAttributeMultiprocessorCount), nothing assumes a whole 256-CU chip:
 *   paper-size geometry   (CUs / 40) * 8 resident groups of five workgroups (decode_pipe.hip), one utterance per group; more
 *                         rows than groups: a group steps two (three) utterances alternately, the shortest rows share
 *                         (rows are assigned longest first); beyond three per group, equal-sized launches;
 *   n_resch > 128         G workgroups per utterance (decode_coop.hip), G * rows <= CUs per launch;
 *   other geometries      one workgroup (one CU) per utterance.
 * Every wait between workgroups is bounded; when a multi-workgroup launch gives up (its workgroups were not co-resident:
 * CU-masked or shared GPU) qpn_decode / qpn_decode_finish re-run the call once with a smaller footprint (one-CU kernels,
 * or half the workgroups per utterance) before returning QPN_ENODEV.
 *   B          batch rows                         n_x   seed samples per row (x is B x n_x)
 *   F          frames of h (h is B x n_aux x F; if upsampling_factor==0, F = samples)
 *   Td         columns of the dilated factors (B x Td), float64 or float32 (d_is_f32)
 *   h_n_samples[B]  samples to generate per row (n_samples_list)
 *   maxd       int(nanmax(ceil(dilated_factors))) over the batch (qpnet.py:347-350)
 *   d_teacher  optional (B x max_n) int64: fed back instead of the pick (teacher forcing)
 *   d_out      (B x max_n) int64 picks, row-major, max_n = max(h_n_samples)
 *   d_logits   optional (B x max_n x n_quantize) fp32 per-step logits
 * Rows are returned in INPUT order; completion-order / list-mutation semantics of the
 * reference are applied by the Python mirror.  Blocks until the stream has finished.
 */
int qpn_decode(qpn_handle* h, int B, int n_x, int64_t F, int64_t Td,
               const int64_t* d_x, const float* d_h, const void* d_dfac, int d_is_f32,
               const int64_t* h_n_samples, int maxd, int mode, uint64_t seed,
               const int64_t* d_teacher, int64_t* d_out, float* d_logits, void* stream);

/* Same, split for stream use: enqueue only enqueues (no host synchronisation: the utterance descriptors are staged in
 * pinned memory owned by the handle) and returns; finish synchronises the stream and returns the device-side status
 * (QPN_ERANGE ...).  One decode in flight per handle: a second enqueue before finish returns QPN_ESTATE; the caller's
 * buffers must stay valid until finish (it may re-run the call, see above). */
int qpn_decode_enqueue(qpn_handle* h, int B, int n_x, int64_t F, int64_t Td,
                       const int64_t* d_x, const float* d_h, const void* d_dfac, int d_is_f32,
                       const int64_t* h_n_samples, int maxd, int mode, uint64_t seed,
                       const int64_t* d_teacher, int64_t* d_out, float* d_logits, void* stream);
int qpn_decode_finish(qpn_handle* h, void* stream);

/* Live output: read finished samples while the decode kernel runs.
 * Arm (every >= 1) or disarm (every == 0) live output for the decode calls enqueued on this handle from now on.  An armed
 * call is the same launch plan with the same results; in addition the kernel mirrors every sample it picks into host memory
 * owned by the handle and publishes, per row, how many are final there: after every `every` samples of the row and after
 * its last one.  Not offered together with teacher forcing or the logits output (an armed enqueue with d_teacher or
 * d_logits returns QPN_EINVAL), and an armed enqueue must not be captured into a HIP graph (it writes the counters from
 * the host).  QPN_ESTATE while a decode is in flight. */
int qpn_decode_live(qpn_handle* h, int every);

/* Sampling controls: temperature and top-k of the draw of QPN_MODE_SAMPLING, for the decode calls enqueued on this handle from now on
 * (sticky, like qpn_decode_live; (1.0f, 0) restores the default draw, which is bit for bit the draw of a handle that never called this).
 * With invT = 1.0f / temperature (fp32, formed here) the class weights are e_c = qexp((l_c - max l) * invT); top_k = k in 1..n_quantize-1
 * keeps the classes whose logit is >= the k-th largest (counted with multiplicity; classes tied with it are all kept) and gives the others
 * weight 0; top_k = 0 or n_quantize keeps every class.  The draw stays the fixed-order inverse-CDF draw with the Philox counter (step, row):
 * reproducible bit for bit on the CPU, the same on every decode kernel, with teacher forcing, the logits output, live
 * output and cancel, and in the re-run after a launch that gave up.  The values travel as kernel arguments.  QPN_MODE_ARGMAX calls ignore
 * them.  Arguments are checked before the device is looked at (works on a handle created without a GPU): QPN_EINVAL naming `temperature`
 * when it is NaN, infinite, <= 0 or so small that 1.0f / temperature is not finite, or `top_k` when it is < 0 or > n_quantize; QPN_ESTATE
 * while a decode is in flight. */
int qpn_decode_sampling(qpn_handle* h, float temperature, int top_k);

/* qpn_decode_sampling with the two cuts that adapt to the width of the distribution; qpn_decode_sampling(h, T, k) is this call with (1.0f, 0.0f),
 * which switches both off.  On the weights e_c above (0 outside the top-k set; the maximum's is exactly 1.0f):
 *   min_p in [0, 1] keeps the classes with e_c >= min_p, i.e. whose probability is at least min_p times the most probable class's (0: off);
 *   top_p in (0, 1] then keeps the classes with e_c >= w*, where w* is the largest weight of the row whose mass S(w*) -- the fixed-order fp32
 *   sum of the weights >= w*, DESIGN.md section 3 -- reaches top_p * S(0): the most probable classes whose mass reaches the fraction top_p of
 *   the whole, classes tied with the last of them all kept (1: off).
 * The draw is then the same fixed-order draw over what is left, reproducible bit for bit on the CPU like the rest, on every decode kernel.  Sticky,
 * kernel arguments, remembered for the re-run of a launch that gave up, ignored by QPN_MODE_ARGMAX, all as above.  Checked before the device is
 * looked at: QPN_EINVAL naming `temperature` / `top_k` as above, `top_p` when it is NaN, <= 0 or > 1, `min_p` when it is NaN, < 0 or > 1;
 * QPN_ESTATE while a decode is in flight. */
int qpn_decode_sampling_ex(qpn_handle* h, float temperature, int top_k, float top_p, float min_p);

/* Per-row sampling: one record per batch row, in the caller's INPUT order (row b of d_x / d_h / h_n_samples), for the QPN_MODE_SAMPLING calls enqueued on
 * this handle from now on (sticky, like qpn_decode_sampling; the array is copied into the handle).  The pick of row b at step i is the controlled draw
 * above with row b's temperature / top_k / top_p / min_p and the uniform of the Philox counter (step i, h_rows[b].stream) under the key h_rows[b].seed:
 * a row's samples depend on its own inputs and its own record only -- not on its row index, the batch size, the launch plan or the kernel (DESIGN.md
 * section 3).  A record with the neutral values (1.0f, 0, 1.0f, 0.0f) draws the bits of the default draw, and the records {s, b, c} in every row b are
 * the uniform call with seed s and controls c.  While records are set, the enqueue's own `seed` and the values of qpn_decode_sampling(_ex) are ignored by
 * QPN_MODE_SAMPLING calls; QPN_MODE_ARGMAX calls ignore the records; an enqueue with B != n_rows returns QPN_EINVAL naming n_rows.  n_rows == 0
 * switches the records off: every later call is the call of a handle that never had any (same kernels, same bytes).  The records in force at the
 * enqueue are remembered with the call (the re-run after a launch that gave up draws with them) and reach the kernels as a small device table that is
 * copied on the call's stream with the utterance descriptors: no host wait.  Teacher forcing, the logits output, live output and cancel compose unchanged.
 * Checked before the device is looked at (works on a handle created without a GPU): QPN_EINVAL for n_rows < 0, a NULL array with n_rows > 0, and per
 * record the rules and messages of qpn_decode_sampling_ex with "row <b>: " in front; QPN_ESTATE while a decode is in flight. */
typedef struct { uint64_t seed; uint32_t stream; float temperature; int32_t top_k; float top_p, min_p; } qpn_row_draw;
int qpn_decode_row_sampling(qpn_handle* h, int n_rows, const qpn_row_draw* h_rows);

/* Frame-rate sampling controls: a draw track, one record per (batch row b, feature frame f), f in [0, n_frames), for the QPN_MODE_SAMPLING calls enqueued on
 * this handle from now on (sticky, like qpn_decode_row_sampling; h_track is a host array, row-major n_rows x n_frames, rows in the caller's INPUT order, copied
 * into the handle).  n_frames is the F of the calls that follow: the frame axis of d_h.  Generated sample i of row b is the controlled draw above with an
 * unchanged uniform and the four values of the record of the frame whose features that step reads,
 *     f(i) = min(F - 1, c(i) / U),  c(i) = n_x - 1 + i,  U = upsampling_factor   (U == 0: f(i) = min(F - 1, c(i))),
 * c(i) being the reference's current_index (qpnet.py:450-451: the un-padded column of the upsampled h that the generation loop indexes; the features
 * are upsampled at qpnet.py:343-344).  Steps over the known prefix draw nothing and use no record.  Key and counter word are those of the call
 * without a track: (call seed, batch row), or the row's (seed, stream) when qpn_decode_row_sampling records are set -- tracks and records compose, the
 * four values of the records are then unused.  Hence, bit for bit: a track holding one record c in every frame of row b gives row b the samples of the
 * per-row call whose record for b holds c; and two tracks that agree on frames [0, f*) of a row give the same samples [0, i*) of it, i* the first i
 * with f(i) >= f*, whatever they hold elsewhere.  QPN_MODE_ARGMAX calls ignore the track.  An enqueue with B != n_rows or
 * F != n_frames returns QPN_EINVAL naming which.  n_rows == 0 switches the track off: every later call is the call of a handle that never had one
 * (same kernels, same bytes).  The table is kept in pinned memory that this call allocates (the enqueue allocates none), reaches the kernels by a copy
 * on the call's stream without a host wait, and stays in force for the re-run after a launch that gave up.  Teacher forcing, the logits output, live
 * output and cancel compose unchanged.  Checked before the device is looked at (works on a handle created without a GPU): QPN_EINVAL for n_rows < 0,
 * n_frames < 1 or a NULL array with n_rows > 0, and per record the rules and messages of qpn_decode_sampling_ex with "row <b> frame <f>: " in front;
 * QPN_ESTATE while a decode is in flight. */
typedef struct { float temperature; int32_t top_k; float top_p, min_p; } qpn_frame_draw;
int qpn_decode_frame_sampling(qpn_handle* h, int n_rows, int64_t n_frames, const qpn_frame_draw* h_track);

/* Non-blocking.  For the decode in flight: h_done[B] = samples of each row (input order) that are final in the mirror;
 * *h_samples / *row_stride = the mirror (int32 sample ids, row b at *h_samples + b * *row_stride; host memory owned by the
 * handle, valid until the next enqueue); *running = 0 once everything the enqueue put on the stream has completed.  The
 * counts never decrease during a call, also not while qpn_decode_finish re-runs a launch that gave up (the re-run produces
 * the same samples bit for bit, so what has been read stays valid).  A launch that gave up leaves *running == 0 with rows
 * short of their n_samples: qpn_decode_finish completes them in d_out.  QPN_ESTATE with no decode in flight or live output
 * not armed for it, QPN_EINVAL for null arguments.  After qpn_decode_cancel, *running drops to 0 with rows short in the same way. */
int qpn_decode_poll(qpn_handle* h, int64_t* h_done, const int32_t** h_samples, int64_t* row_stride, int* running);

/* Non-blocking: ask the decode in flight to stop.  One store to host memory that the kernels read -- no stream work, no host wait.
 * Every row stops at a publish point of its own: the next one after the request has become visible to the device, or the one after
 * that (the kernel looks at the word it fetched at the previous publish point, so that no step waits for host memory).  Rows of a
 * later launch of the plan, and launches that start after the request, publish nothing.  A row's published count is final and never
 * decreases; samples [0, count) of the row are valid in d_out and in the mirror and are bit for bit what the uncancelled call
 * produces there; anything at or beyond the count is unspecified.  qpn_decode_finish then returns as soon as the launches have
 * drained: it never re-runs a call with a request (neither one that stopped on it nor one whose launch had given up before), does
 * not report the drain as QPN_ENODEV, and returns QPN_OK -- or QPN_ERANGE if a tap left its ring before the stop.  A cancelled call
 * is over: nothing of it carries into the next call.  Idempotent (a second request is QPN_OK); a request that arrives after the
 * kernels have ended is QPN_OK and changes nothing.  QPN_ESTATE with no decode in flight, or when the call in flight was enqueued
 * without live output (only armed calls have publish points; unarmed calls run as they always did).  The handle's thread rule is
 * unchanged: one thread at a time per handle. */
int qpn_decode_cancel(qpn_handle* h);

/* After qpn_decode_finish of an armed call, until the next enqueue: h_done[B] = the final count of each row (input order) --
 * n_samples[b] for every row of a call that ran to its end; *cancelled = 1 exactly when a stop was requested (qpn_decode_cancel)
 * and at least one row ended short.  QPN_ESTATE while a decode is in flight or when the last call was not armed, QPN_EINVAL for
 * null arguments. */
int qpn_decode_final_counts(qpn_handle* h, int64_t* h_done, int* cancelled);

/* Device time (ms) of the persistent decode kernel of the last finished qpn_decode call,
 * measured with HIP events on the launch stream (bench.py roofline). */
float qpn_last_decode_kernel_ms(qpn_handle* h);

/* The launch plan of the last decode call as text, e.g. "pipe rows=96 waves=1 x 96 (2 per group); one-cu rows=0"
 * (diagnostics / bench.py; owned by the handle, valid until the next decode call). */
const char* qpn_last_decode_plan(qpn_handle* h);

/* The launch plan a decode call of B utterances would follow, as the text qpn_last_decode_plan shows after it: attempt 0 = the
 * first plan, attempt 1 = what qpn_decode_finish runs after a launch of that plan gave up (the text behind "retried: "), or
 * QPN_ESTATE where no retry exists.  Host arithmetic only: works on a handle created without a GPU.  n_cus > 0 plans for a
 * device of that many compute units (its pipelined launches hold (n_cus / 40) * 8 groups); n_cus <= 0 means the handle's own
 * device (QPN_ENODEV without one).  Geometry and knobs are the handle's (the environment as read by qpn_create); the call's
 * pitch-tap rings are taken to be short enough for the batched cooperative kernel's 32-bit offsets (any maxd below thousands). */
int qpn_decode_plan_query(qpn_handle* h, int n_cus, int B, int attempt, char* buf, size_t cap);

/*
 * QPNet.forward (reference src/nets/qpnet.py:239-312), teacher forced, fused fp32-MFMA kernels.
 *   d_flat   flat fp32 parameters (state_dict order), read at call time (training updates them)
 *   d_x      (B x T) int64 samples         d_h  (B x n_aux x F) fp32 frame-rate features
 *   d_dfac   (B x Td) fp32 dilated factors BL   batch_length (same for every row, qpnet.py:253)
 *   maxd     int(max(ceil(dilated_factors))) over the whole tensor (qpnet.py:255)
 *   d_logits (B x BL x n_quantize) fp32 out.  Activations needed by backward stay in the
 *   handle's workspace until the next qpn_train_forward.  Asynchronous on `stream`.
 */
int qpn_train_forward(qpn_handle* h, const float* d_flat, int B, int64_t T, int64_t F, int64_t Td, int BL, int maxd,
                      const int64_t* d_x, const float* d_h, const float* d_dfac, float* d_logits, void* stream);

/* autograd of the above (reference: loss.backward(), src/bin/qpnet_train.py:529-530):
 * d_dlogits (B x BL x n_quantize) -> d_flatgrad (n_params, overwritten), same layout as d_flat. */
int qpn_train_backward(qpn_handle* h, const float* d_dlogits, float* d_flatgrad, void* stream);

/* Same with the data-parallel hooks of the one gradient exchange per step (replaces the reference's dead DataParallel wrapper,
 * src/bin/qpnet_train.py:416-423): the flat gradient is multiplied by grad_scale (the rank's row count B*BL) inside the
 * reduction kernel; with append_scale != 0, d_flatgrad must hold n_params + 4 floats and receives {grad_scale, flagged, 0, 0} behind
 * the gradient, so ONE all-reduce(SUM) carries sum_r n_r g_r, sum_r n_r and the number of ranks whose device-side status word is set
 * (flagged = 1.0 then: qpn_adam_step_ex skips the update on EVERY rank).  append_scale = 1: the backward's last launch writes the flag (it then covers the
 * backward's own status bits too); 2: the trailer leaves with the early exchange bucket (qpn_train_early_bucket) and carries the forward's bits only. */
int qpn_train_backward_ex(qpn_handle* h, const float* d_dlogits, float* d_flatgrad, float grad_scale, int append_scale, void* stream);

/* Arm (d_dh != NULL) or disarm (NULL) the feature gradient for the NEXT backward enqueued on this handle: qpn_train_backward[_ex], or the one inside
 * qpn_train_step* / qpn_train_step_acc.  That backward also writes d_dh[B][n_aux][F] = d(sum(dlogits * logits)) / d h of its forward (F as that forward was
 * given it; for the fused step: d(mean CE of this chunk) / dh, not weighted by grad_scale), every element, exact zeros where no row reaches (the frames in
 * front of the chunk's receptive field; with upsampling_factor = 0 the leading F - (rows of the chunk) columns).  One shot:
 * consumed by that backward.  n must equal B * n_aux * F of the forward the backward belongs to, else that backward returns QPN_EINVAL naming n before
 * it launches anything (and the arm is dropped).  Reads the weights as they are when the backward runs (before the step's Adam launch).
 * The gradient with respect to the dilated factors is not computed: the pitch tap is a rounding, its derivative is zero almost everywhere (what the
 * reference's autograd yields too).  Fixed summation order, no atomics of its own; where the layer backward's accumulators it reads are float atomics (the
 * frame-rate aux path, the pitch-adaptive layers' scatter) the result is reproducible to rounding, not bit for bit.
 * Arguments are checked before the device is looked at (works on a handle created without a GPU): QPN_EINVAL for a null handle, or n < 1 with a
 * non-null d_dh; disarming always succeeds.  An armed backward enqueued while its stream is capturing returns QPN_ESTATE (the arm is host state that a
 * replay would not renew) and drops the arm.  A backward that is not armed launches exactly what it always launched. */
int qpn_train_input_grad(qpn_handle* h, float* d_dh, int64_t n);

/* Number of qpn_train_forward calls on this handle so far.  The activations backward needs live in the handle's workspace
 * (one outstanding forward per handle): a caller that defers backward (torch autograd) records the value after forward and
 * compares before backward (reference: autograd keeps per-call activations, src/bin/qpnet_train.py:520-530). */
int64_t qpn_train_generation(qpn_handle* h);

/* What the handle's latest training calls launched, as text: "fwd[...] launches" of the latest forward and, behind " | ", "bwd[...] jobs" of its backward
 * once that has run -- the layer path of each direction (generic / persist / stack), the fused forms, every launch with (grid; block; dynamic LDS bytes),
 * the backward's jobs in order with their stream (main: / side:) and the fork / mid / join / wait / early event edges.  Diagnostics and tests; built when
 * asked for (a step formats nothing), owned by the handle, valid until the next training call; "" before the first forward. */
const char* qpn_train_last_plan(qpn_handle* h);

/* Synchronise and report the device-side status of the last training call (QPN_ERANGE when a
 * pitch-dependent tap left its layer input: reference assert qpnet.py:294). */
int qpn_train_status(qpn_handle* h, void* stream);

/* The same check without draining the stream: _enqueue copies the status word (sticky: kernels OR into it, only a read
 * clears it) to pinned memory behind the work enqueued so far and returns; _collect waits for that copy alone and
 * reports it.  The module calls _collect at the start of a forward and _enqueue behind it: an out-of-range tap of
 * step i is raised at step i+1 (reference: assert at step i, qpnet.py:294), and no step is serialised for it.
 * A word that is reported is cleared with a memset on the stream of the handle's latest training call -- a qpn_train_step* call that
 * finds it: on that call's own stream, in front of the step run on it next.  A caller that moves a handle from one stream to another
 * orders the two itself (the step reads what the step before it wrote). */
int qpn_train_status_enqueue(qpn_handle* h, void* stream);
int qpn_train_status_collect(qpn_handle* h);
/* ... every enqueued check EXCEPT the newest one: never waits for the work the device still has queued (a fused training loop calls it
 * at the start of every step and reports a bad chunk two steps late at most; reference: the in-line asserts of qpnet.py:294, qpnet_train.py:525). */
int qpn_train_status_collect_lagged(qpn_handle* h);
/* The same without ever waiting: only the checks whose copies have already landed are reported (hipEventQuery); *pending (may be NULL)
 * receives the number still in flight.  For callers that must not stall the host behind queued work (QPNet.status_check = "lazy"). */
int qpn_train_status_poll(qpn_handle* h, int* pending);

/* torch.nn.CrossEntropyLoss() (mean) on the logits above and, optionally, its gradient
 * (reference src/bin/qpnet_train.py:430,526-528; a target outside [0, n_quantize) is clamped and flagged: qpn_train_status
 * returns QPN_ERANGE, the reference asserts at :525).  d_targets is the (B x tgt_stride) int64 target
 * tensor whose LAST BL columns are used (batch_t[:, -batch_length:]).  h_loss (optional, host)
 * receives the loss (synchronises); d_dlogits (optional) receives dL/dlogits. */
int qpn_ce_loss(qpn_handle* h, const float* d_logits, const int64_t* d_targets, int64_t tgt_stride, int B, int BL,
                float* d_dlogits, double* h_loss, void* stream);

/* Knowledge distillation (Hinton-style soft targets; DESIGN.md section 5, "Soft-target loss"): the counterpart of qpn_ce_loss for logits the caller
 * provides.  Per row, with z = d_logits, t = d_teacher (both B x BL x n_quantize fp32), y the hard target (d_targets / tgt_stride as in qpn_ce_loss):
 *   L_row = (1 - alpha) CE(z, y) + alpha T^2 KL(softmax(t / T) || softmax(z / T))
 *   dL/dz = (1 - alpha) (softmax(z) - onehot(y)) + alpha T (softmax(z / T) - softmax(t / T))
 * The loss is the mean of L_row over the B * BL rows and d_dlogits (optional) receives dL/dz over the row count, as qpn_ce_loss does; the CE term is that
 * call's arithmetic, target rule included (out of range: clamped and flagged).  One kernel (k_ce_distill), fixed reduction order:
 * d_dlogits is the same bits from run to run.  h_loss3 (optional, host; synchronises) receives {the loss, the hard CE mean, the T^2 KL mean}; without it the
 * loss stays on the device for qpn_train_loss / qpn_train_loss_enqueue.  A NaN or an infinity in a row of d_teacher sets bit 5 (1 << 5) of the training status word:
 * the next status report returns QPN_ERANGE ("... teacher logits ..."), an Adam launch that finds the word set skips its update as for every other bit.
 * Arguments are checked before the device is looked at (works on a handle created without a GPU), QPN_EINVAL naming the argument: a null handle or pointer,
 * B < 1, BL < 1, tgt_stride < BL, alpha outside (0, 1] or NaN, temperature <= 0, NaN or infinite; with n_quantize a multiple of 256 the three float
 * buffers must be 16-byte aligned. */
int qpn_distill_loss(qpn_handle* h, const float* d_logits, const float* d_teacher, const int64_t* d_targets, int64_t tgt_stride, int B, int BL,
                     float alpha, float temperature, float* d_dlogits, double* h_loss3, void* stream);

/* Arm (d_teacher != NULL) or disarm (NULL) the soft-target loss above for the NEXT forward-with-loss enqueued on this handle: qpn_train_forward_loss, or the
 * one inside qpn_train_step / _clip / _avg / _acc.  That forward computes qpn_distill_loss(its logits, d_teacher, its targets, alpha, temperature) in the place
 * of the cross entropy: its loss (qpn_train_loss, the step's h_loss) is the distillation total and its d_dlogits that loss's gradient, which the backward
 * then takes as ever.  One shot: consumed by that forward; a plain qpn_train_forward computes no loss and leaves the arm alone.  An armed forward takes the
 * route QPN_CE_SEPARATE=1 selects -- the forward writes the logits, k_ce_distill runs in k_ce's place, the backward computes the post-net itself -- on every
 * training path; d_teacher is read when that kernel runs.  n must equal B * BL * n_quantize of that forward, else it returns QPN_EINVAL naming n before it
 * launches anything (and the arm is dropped); an armed forward enqueued while its stream is capturing returns QPN_ESTATE (the arm is host state that a
 * replay would not renew) and drops the arm.  Arguments are checked before the device is looked at (works on a handle created without a GPU), QPN_EINVAL
 * naming the argument: a null handle, n < 1 with a non-null d_teacher, alpha outside (0, 1] or NaN, temperature <= 0, NaN or infinite, a d_teacher that is
 * not 16-byte aligned; disarming always succeeds.  A forward that is not armed launches exactly what it always launched. */
int qpn_train_distill(qpn_handle* h, const float* d_teacher, int64_t n, float alpha, float temperature);

/* Loss options ("Loss options"): what a user of torch.nn.CrossEntropyLoss configures -- per-row sample weights, ignore_index,
 * label_smoothing, and what the sum is divided by.  Per row r = (b, t) with logits z (Q = n_quantize classes) and target y:
 *   w_r   = d_weights[r]  (1 when d_weights is NULL);   w_r = 0 when use_ignore and y == ignore_index
 *   CE_r  = lse(z) - (1 - eps) z_y - (eps / Q) sum_q z_q                      eps = label_smoothing in [0, 1)
 *   g_r   = softmax(z) - (1 - eps) onehot(y) - eps / Q
 *   L     = (1 / N) sum_r w_r CE_r        dL/dz_r = (w_r / N) g_r
 *   N     = B * BL   for norm = 0 ("rows");    N = sum_r w_r   for norm = 1 ("weights": torch's `mean` with ignore_index)
 * CE_r is torch.nn.functional.cross_entropy(..., label_smoothing=eps, reduction="none").  A row with w_r == 0 contributes nothing: its logits are not read, its
 * target is not range-checked (padding may hold anything), its d_dlogits row is exact +0.  A weight that is NaN, infinite or negative counts as 0 and sets
 * value 64 (1 << 6) of the training status word: the next status report returns QPN_ERANGE ("... sample weights ..."), an Adam launch that finds the word set
 * skips its update as for every other bit.  norm = 1 with sum_r w_r == 0: the loss is 0, d_dlogits all zeros, no flag.  With norm = 0 the per-chunk loss stays
 * a mean over the row count, so the row-weighted combination over ranks and accumulation windows gives sum w CE / sum rows exactly; norm = 1 is for updates that
 * one chunk forms.
 * Bitwise: k_ce_opt keeps k_ce's arithmetic and reduction order and forms the row's scale w_r / N once, in fp32: with all weights 1, eps 0, norm 0 its d_dlogits
 * is qpn_ce_loss's bit for bit; with a power-of-two weight a row is exactly that weight times qpn_ce_loss's row.  The effective sum of weights that norm = 1
 * divides by is computed in fp64 in a fixed order (k_weight_mass): d_dlogits is the same bits from run to run for both norms. */
typedef struct { const float* d_weights; int64_t n_weights; int use_ignore; int64_t ignore_index;
                 float label_smoothing; int norm; /* 0 rows, 1 weights */ } qpn_loss_opts;

/* qpn_ce_loss with the options above (one kernel, k_ce_opt; norm = 1: k_weight_mass in front of it).  d_weights: B x BL fp32, contiguous, n_weights == B * BL.
 * h_loss2 (optional, host; synchronises) receives {the loss, the effective sum of weights}; without it the loss stays on the device for qpn_train_loss.
 * Arguments are checked before the device is looked at (works on a handle created without a GPU), QPN_EINVAL naming the argument: a null handle or pointer
 * (opts included), B < 1, BL < 1, tgt_stride < BL, n_weights < 1 or != B * BL with weights, label_smoothing NaN or outside [0, 1), norm outside {0, 1},
 * d_weights not 4-byte aligned; with n_quantize a multiple of 256, d_logits and d_dlogits must be 16-byte aligned. */
int qpn_ce_loss_opts(qpn_handle* h, const float* d_logits, const int64_t* d_targets, int64_t tgt_stride, int B, int BL,
                     const qpn_loss_opts* opts, float* d_dlogits, double* h_loss2, void* stream);

/* qpn_distill_loss with row weights and ignore_index: w_r multiplies the whole row loss, CE term and KL term alike, and N divides both.  label_smoothing > 0 is
 * refused (QPN_EINVAL naming label_smoothing: the soft targets already smooth).  Otherwise the arguments and checks of qpn_distill_loss and qpn_ce_loss_opts.
 * With all weights 1 and norm 0, d_dlogits is qpn_distill_loss's bit for bit; a power-of-two weight scales a row exactly.  h_loss4 (optional, host;
 * synchronises): qpn_distill_loss's three values, then the effective sum of weights. */
int qpn_distill_loss_opts(qpn_handle* h, const float* d_logits, const float* d_teacher, const int64_t* d_targets, int64_t tgt_stride, int B, int BL,
                          float alpha, float temperature, const qpn_loss_opts* opts, float* d_dlogits, double* h_loss4, void* stream);

/* Arm (opts != NULL) or disarm (NULL) the loss options for the NEXT forward-with-loss enqueued on this handle, by the rules of qpn_train_distill: one shot,
 * consumed by qpn_train_forward_loss and by the forward inside qpn_train_step / _clip / _avg / _acc, left alone by a plain qpn_train_forward, dropped by a
 * failing step.  The struct is copied; d_weights is read when the loss kernel runs.  An armed forward takes the route QPN_CE_SEPARATE=1 selects, k_ce_opt in
 * k_ce's place, on every training path; with a distillation arm on the same forward, k_ce_distill's weighted form runs; qpn_train_input_grad composes as ever.
 * n_weights must equal B * BL of that forward, else it returns QPN_EINVAL naming n_weights before it launches anything (and the arm is dropped); an armed
 * forward enqueued while its stream is capturing returns QPN_ESTATE and drops the arm.  A struct that is entirely default (no weights, no ignore, eps 0,
 * norm 0) arms nothing: the next forward launches exactly what it always launched.  Arguments are checked before the device is looked at, QPN_EINVAL naming
 * the argument as for qpn_ce_loss_opts, and label_smoothing > 0 while a teacher is armed (or a teacher armed behind it); disarming always succeeds. */
int qpn_train_loss_opts(qpn_handle* h, const qpn_loss_opts* opts);

/* Forward + loss in one call: qpn_train_forward followed by qpn_ce_loss (reference src/bin/qpnet_train.py:520-528:
 * `batch_output = model(...)`, `criterion(batch_output[i], batch_t[i])`), with the cross entropy and its gradient computed
 * inside the post-net kernel while a tile's logits are still in LDS (paper-size stacks; wider ones run the separate kernel
 * behind the forward -- same results either way).  d_targets / tgt_stride / d_dlogits as in qpn_ce_loss.  d_logits must be a
 * (B x BL x n_quantize) buffer; with want_logits bit 0 clear the implementation may leave it unwritten.  want_logits bit 1
 * (QPN_FWD_BACKWARD_FOLLOWS = 2): the caller promises to run qpn_train_backward[_ex] of this forward next, with this same
 * d_dlogits untouched -- the post-net's backward may then run inside the forward's launch sequence (one kernel for both
 * directions of a row tile); a backward with another buffer, or a repeated one, still computes everything itself.  The loss
 * stays on the device until qpn_train_loss (synchronises) is called. */
#define QPN_FWD_BACKWARD_FOLLOWS 2
int qpn_train_forward_loss(qpn_handle* h, const float* d_flat, int B, int64_t T, int64_t F, int64_t Td, int BL, int maxd,
                           const int64_t* d_x, const float* d_h, const float* d_dfac, const int64_t* d_targets, int64_t tgt_stride,
                           float* d_logits, int want_logits, float* d_dlogits, void* stream);
int qpn_train_loss(qpn_handle* h, double* h_loss, void* stream);
/* The same number without draining the stream at every step (the reference reads loss.item() per step, src/bin/qpnet_train.py:533, and
 * only ever uses the values summed over a reporting interval, :536-541): _enqueue copies this step's loss to pinned memory behind the
 * step's kernels; _collect(newest = 0) returns the one enqueued ONE call earlier (finished long ago: no wait in practice), newest = 1 the
 * last one (waits for it).  *h_valid = 0 when there is no such copy (first step, or already collected). */
int qpn_train_loss_enqueue(qpn_handle* h, void* stream);
int qpn_train_loss_collect(qpn_handle* h, int newest, double* h_loss, int* h_valid);

/* torch.optim.Adam step (reference src/bin/qpnet_train.py:426-429,531), fp32, in place:
 * d_flat, d_m, d_v (n floats each) updated from d_grad; `step` is the 1-based step count. */
int qpn_adam_step(qpn_handle* h, float* d_flat, const float* d_grad, float* d_m, float* d_v, int64_t n,
                  int step, float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* Same, reading the gradient as d_grad[i] / d_grad_denominator[0] (device scalar, e.g. the summed row count behind an
 * all-reduced gradient; NULL = 1): no host read-back and no extra elementwise launch in a data-parallel step.  Non-NULL: d_grad_denominator[1] is the
 * exchanged trailer's flag count (qpn_train_backward_ex): > 0 skips the update, as the handle's own status word does. */
int qpn_adam_step_ex(qpn_handle* h, float* d_flat, const float* d_grad, float* d_m, float* d_v, int64_t n,
                     int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                     const float* d_grad_denominator, void* stream);

/* Gradient-norm clipping inside the optimiser step (no reference counterpart in the trainer itself; the reference-side loop a user writes is
 * `torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)` followed by `Adam.step()`, and this is exactly that pair):
 *   total = sqrt(sum_i g_i^2) over the first n floats of d_grad (/ d_grad_denominator[0] when given: the norm of the AVERAGED gradient), accumulated in fp64 in
 *           a fixed order without atomics -- the same bits from run to run and on every data-parallel rank;
 *   coef  = min(1, max_grad_norm / (total + 1e-6)), computed in fp64 and rounded once to fp32;
 *   g_i  <- (g_i / denominator) * coef, before the weight-decay term; the rest of the update is qpn_adam_step_ex's.  d_grad itself is not modified.
 * max_grad_norm <= 0: exactly qpn_adam_step_ex (qpn_adam_step and qpn_adam_step_ex are this call with 0).  One extra kernel launch per step, no copy, no host wait.
 * A non-finite total (an inf or NaN in the gradient) is reported like the other device-side status bits: the update is skipped (weights, both moments and the
 * applied-update count stay), bit 16 of the sticky status word is set, and the next status report returns QPN_ERANGE ("non-finite gradient norm"). */
int qpn_adam_step_clip(qpn_handle* h, float* d_flat, const float* d_grad, float* d_m, float* d_v, int64_t n,
                       int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                       const float* d_grad_denominator, float max_grad_norm, void* stream);
/* The norm (`total` above) of the LATEST Adam launch on this handle; *h_valid = 0 when that launch did not clip or there was none.  Drains `stream`. */
int qpn_train_grad_norm(qpn_handle* h, double* h_norm, int* h_valid, void* stream);
/* The same without a wait of its own, for a lagged loop: the norm of the step whose loss the last qpn_train_loss_collect returned (behind a clipping launch
 * qpn_train_loss_enqueue takes the norm out in the loss's copy).  *h_valid = 0 when that step did not clip or no loss was returned. */
int qpn_train_grad_norm_lagged(qpn_handle* h, double* h_norm, int* h_valid);

/* Averaged weights (an exponential moving average of the parameters, what WaveNet-family vocoders are decoded with) kept by the optimiser launch itself:
 * the thread that has just computed element i's new weight w_new also does, in fp32,
 *   d_ema[i] <- d_ema[i] + (w_new - d_ema[i]) * (1.0f - ema_decay)          (1.0f - ema_decay is formed once on the host, in fp32)
 * -- no second pass, no extra launch, copy or host wait.  d_ema: n floats, caller-owned and caller-initialised (a copy of the weights is the usual seed);
 * 0 < ema_decay < 1.  d_ema = NULL with ema_decay = 0: exactly qpn_adam_step_clip (qpn_adam_step, _ex and _clip are this call with NULL, 0, and launch the
 * kernels they always did).  Anything else -- a NaN decay, a decay outside (0, 1), or only one of the two given -- returns QPN_EINVAL naming the argument, before the
 * device or the handle's state is looked at.  Skip rule: a skipped update (the sticky status word set, a peer rank's flag in d_grad_denominator[1], or a
 * non-finite clipping norm) leaves d_ema untouched together with the weights, both moments and the applied-update count: the average is of APPLIED states.
 * Weights, moments, reports, norm word and applied-update count are bit for bit those of the call without d_ema; gradient-norm clipping and the
 * data-parallel denominator compose with it unchanged.  Nothing is stored on the handle: the pointer is used by this call's launch only. */
int qpn_adam_step_avg(qpn_handle* h, float* d_flat, const float* d_grad, float* d_m, float* d_v, int64_t n,
                      int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                      const float* d_grad_denominator, float max_grad_norm, float* d_ema, float ema_decay, void* stream);

/* Parameter groups of the optimiser step: a learning rate and a weight decay per range of the flat vector, and ranges that are not updated at all (frozen) --
 * what torch.optim.Adam is given as several param_groups, or by leaving tensors out.  Segment s covers [h_seg_end[s-1], h_seg_end[s]) (h_seg_end[-1] = 0) and belongs
 * to group h_seg_group[s] in [0, n_groups) or is QPN_ADAM_FROZEN.  Sticky on the handle, like qpn_decode_sampling: from this call on EVERY Adam launch of the handle
 * (qpn_adam_step, _ex, _clip, _avg, qpn_train_step, _clip, _avg, the closing micro-step of qpn_train_step_acc) updates element i of a segment of group q with
 * (h_lr[q], h_weight_decay[q]) -- bit for bit what the launch without groups writes there when called with those two values, data-parallel denominator and clip
 * coefficient included; the launch's own lr / weight_decay are ignored, everything else (betas, eps, step, denominator, clipping, averaging) is the call's.  A frozen
 * element's weight, moments and gradient are neither written nor (the averaged weights aside: they go on moving towards the weight that stays) read.  The clipping
 * norm is that of the elements that are not frozen -- bit for bit the norm reported for the same gradient with the frozen elements set to +0, so a non-finite value in
 * a frozen element's gradient does not skip the step.  Reports, status word, applied-update count and the skip rule are unchanged.  A launch whose n is not
 * h_seg_end[n_seg - 1] returns QPN_EINVAL.
 * The group values travel as kernel arguments; only the segment table (adjacent segments of one group merged, plus a pair of ints per 256 elements) lives in device memory.
 * A call whose segment table equals the one the handle holds touches no device memory and only replaces the values: the per-step path of a learning-rate schedule.  A
 * changed table is a set-up call: it may synchronise `stream`, and returns QPN_ESTATE while that stream is capturing.  The arrays are not referenced after return.
 * n_groups = 0 switches groups off: the other arguments are ignored, no device is needed, and every launch is exactly what it was.
 * Errors, checked before the device is looked at (also on a handle created without a GPU), QPN_EINVAL naming the argument: n_groups outside [0, QPN_ADAM_MAX_GROUPS];
 * with n_groups > 0 a NULL array; an h_lr / h_weight_decay that is NaN, infinite or negative (0 is allowed, as in torch); n_seg < 1 or > 2^20; h_seg_end[0] < 1 or
 * h_seg_end not strictly ascending; a group outside [-1, n_groups); no trainable segment.  A valid call without a GPU returns QPN_ENODEV. */
#define QPN_ADAM_MAX_GROUPS 8
#define QPN_ADAM_FROZEN (-1)
int qpn_adam_groups(qpn_handle* h, int n_groups, const float* h_lr, const float* h_weight_decay,
                    int64_t n_seg, const int64_t* h_seg_end, const int32_t* h_seg_group, void* stream);

/* Adam updates APPLIED on this handle so far, counted on the device: a k_adam launch that finds the sticky status word set -- or, behind a data-parallel
 * exchange, a peer rank's flag in the trailer (d_grad_denominator[1] > 0) -- applies nothing (every rank skips a step ANY rank flagged; the others report
 * "a peer rank flagged ..." with QPN_ERANGE).  Drains `stream`.  A caller that keeps the bias correction's step number on the host (the reference:
 * torch.optim.Adam's state["step"], src/bin/qpnet_train.py:531) re-bases it on this count after a status error. */
int qpn_train_applied_updates(qpn_handle* h, int64_t* applied, void* stream);

/* One optimisation step of the reference's training loop (src/bin/qpnet_train.py:517-531: forward, CrossEntropyLoss, backward, Adam.step, loss.item())
 * behind ONE call: qpn_train_forward_loss + qpn_train_backward + qpn_adam_step and the loss / status bookkeeping, in that order, so that the host side of
 * a step is a single foreign call.  d_logits / d_dlogits: caller-owned B*BL*n_quantize floats (the logits are not written); d_grad: n (+ 4) floats.
 * loss_mode 0: none; 1: "lagged" -- this step's loss is copied out behind its kernels, *h_loss receives the previous step's (*h_valid = 0 when there is none;
 * qpn_train_loss_collect(newest = 1) fetches the last one), the stream is never drained; 2: this step's loss, read in the call.  The device-side status word
 * (a tap or target out of range) is reported two steps late at most in modes 0 / 1, in the call in mode 2; flagged steps do not touch the parameters. */
int qpn_train_step(qpn_handle* h, float* d_flat, int B, int64_t T, int64_t F, int64_t Td, int BL, int maxd,
                   const int64_t* d_x, const float* d_h, const float* d_dfac, const int64_t* d_targets, int64_t tgt_stride,
                   float* d_logits, float* d_dlogits, float* d_grad, float* d_m, float* d_v, int64_t n,
                   int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                   int loss_mode, double* h_loss, int* h_valid, void* stream);

/* qpn_train_step with qpn_adam_step_clip as its optimiser step (max_grad_norm <= 0: exactly qpn_train_step, which is this call with 0 and NULL).  *h_grad_norm
 * (may be NULL) is delivered with *h_loss: loss_mode 1 -- the previous step's norm, valid exactly when *h_valid is set (it comes out of the same pinned slot; after the
 * last step qpn_train_loss_collect(newest = 1) + qpn_train_grad_norm_lagged fetch the pair); 2 -- this step's; 0 -- none.  The norm launch counts towards QPN_PG_ADAM. */
int qpn_train_step_clip(qpn_handle* h, float* d_flat, int B, int64_t T, int64_t F, int64_t Td, int BL, int maxd,
                        const int64_t* d_x, const float* d_h, const float* d_dfac, const int64_t* d_targets, int64_t tgt_stride,
                        float* d_logits, float* d_dlogits, float* d_grad, float* d_m, float* d_v, int64_t n,
                        int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                        int loss_mode, double* h_loss, int* h_valid, float max_grad_norm, double* h_grad_norm, void* stream);

/* qpn_train_step_clip with qpn_adam_step_avg as its optimiser step: d_ema / ema_decay as there (NULL, 0: exactly qpn_train_step_clip, which is this call with
 * NULL, 0); every loss_mode moves the average. */
int qpn_train_step_avg(qpn_handle* h, float* d_flat, int B, int64_t T, int64_t F, int64_t Td, int BL, int maxd,
                       const int64_t* d_x, const float* d_h, const float* d_dfac, const int64_t* d_targets, int64_t tgt_stride,
                       float* d_logits, float* d_dlogits, float* d_grad, float* d_m, float* d_v, int64_t n,
                       int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                       int loss_mode, double* h_loss, int* h_valid, float max_grad_norm, double* h_grad_norm,
                       float* d_ema, float ema_decay, void* stream);

/* Gradient accumulation (no reference counterpart: the reference trainer applies one Adam update per chunk): the gradient of SEVERAL chunks behind one update, as the
 * sum a data-parallel step takes over ranks, taken over time.  d_acc[i] = first ? d_grad[i] : d_acc[i] + d_grad[i] for i < cnt -- callers pass n_params + 4: the
 * row-weighted gradient n_r * g_r that qpn_train_backward_ex(grad_scale = n_r, append_scale = 1) left, and its trailer {n_r, flagged_r, 0, 0}.  Plain fp32, one add per
 * element, no atomics: the same bits from run to run and on every rank.  first != 0 overwrites without reading d_acc (it needs no clearing; NaNs in it do not survive).
 * qpn_adam_step_avg(d_grad = d_acc, d_grad_denominator = d_acc + n_params) then applies the update of the mean over all the window's rows, and skips it when any of its
 * chunks was flagged.  Errors (QPN_EINVAL naming the argument, before the device is looked at): a NULL pointer, cnt < 1, d_acc == d_grad. */
int qpn_grad_accumulate(qpn_handle* h, float* d_acc, const float* d_grad, int64_t cnt, int first, void* stream);

/* qpn_train_step_avg as micro-step `micro` (0-based) of a window of `micro_count` chunks, still ONE call per chunk.  micro_count > 1: every micro-step enqueues
 * qpn_train_forward_loss (QPN_FWD_BACKWARD_FOLLOWS), qpn_train_backward_ex(grad_scale = B * BL, append_scale = 1) into d_grad and qpn_grad_accumulate(d_acc, d_grad, n + 4,
 * first = (micro == 0)); only micro == micro_count - 1 also enqueues qpn_adam_step_avg with d_grad = d_acc, d_grad_denominator = d_acc + n and the given max_grad_norm,
 * d_ema, ema_decay.  d_grad (n + 4 floats) holds this micro-step's row-weighted gradient and trailer afterwards; d_acc: n + 4 caller-owned floats, not d_grad.
 * `step` is the 1-based UPDATE number, the same for every micro-step of a window.  loss_mode, *h_loss, *h_valid as in qpn_train_step: every micro-step has a loss of its
 * own.  *h_grad_norm comes only with the loss of a window-closing micro-step (the others ran no norm launch: qpn_train_grad_norm_lagged's "that step did not clip" rule).
 * A micro-step in front of the closing one has no Adam launch; its last kernel, the accumulate, carries the status word and the loss partials to pinned memory instead.
 * Skip rule: a flagged micro-step leaves its flag in the trailer, the flags are summed into d_acc[n + 1], and the closing Adam launch skips through its own sticky
 * status word or that sum: weights, both moments, the average, the norm word's meaning and the applied-update count stay as the last clean update left them, and the
 * status report is QPN_ERANGE.  d_acc = NULL, micro = 0, micro_count = 1: exactly qpn_train_step_avg.  Errors (QPN_EINVAL naming the argument, before the averaged-weights
 * checks, the device and the handle's state): micro_count < 1, micro outside [0, micro_count), d_acc == NULL with micro_count > 1, d_acc == d_grad. */
int qpn_train_step_acc(qpn_handle* h, float* d_flat, int B, int64_t T, int64_t F, int64_t Td, int BL, int maxd,
                       const int64_t* d_x, const float* d_h, const float* d_dfac, const int64_t* d_targets, int64_t tgt_stride,
                       float* d_logits, float* d_dlogits, float* d_grad, float* d_m, float* d_v, int64_t n,
                       int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                       int loss_mode, double* h_loss, int* h_valid, float max_grad_norm, double* h_grad_norm,
                       float* d_ema, float ema_decay, float* d_acc, int micro, int micro_count, void* stream);

/* Per-tensor training statistics (no reference counterpart; the loop a user writes is 3 x n_tensors torch.norm launches on views of the flat buffers): for every
 * tensor t = elements [h_tensor_end[t-1], h_tensor_end[t]) of the flat vectors (h_tensor_end[-1] = 0; state_dict order is the layout of d_flat), one record
 *   grad_sumsq     sum of (g_i / den)^2 over the tensor's FINITE gradient elements, den = d_grad_denominator[0] (the summed row count of a data-parallel or accumulated
 *                  gradient: what the Adam launch divides by; must be > 0) or 1 when NULL;   grad_absmax: max |g_i / den| over them;   grad_nonfinite: the NaN / inf among them
 *   weight_sumsq   sum of w_i^2 over the finite weights;   weight_absmax: max |w_i| over them
 *   update_sumsq   sum of u_i^2, u_i = m_i / (sqrtf(v_i) / bc2_sqrt + eps) in the fp32 operations of the Adam kernel, bc2_sqrt that of update number `step`
 * computed by two launches that only READ: the Adam launch leaves d_grad as it is, and d_m, d_v after it determine what it subtracted from the weights,
 * (lr / bc1) * u_i -- sqrt(update_sumsq) * lr / bc1 with the lr of the tensor's group is the norm of the latest update, nothing of which was stored (bc1 = 1 - beta1^step,
 * formed in fp64 and rounded once to fp32, as the launch forms it).  After a skipped update m and v are those of the last applied one: so is the record.
 * Sums are fp64 (an fp32 square is exact in it) in ONE fixed order without atomics, a function of the table alone: the same bits from run to run, at any alignment
 * of the four bases (16-byte loads where a base allows, four loads otherwise) and on every data-parallel rank.
 * d_grad may be NULL: the gradient fields are 0 (d_grad_denominator is not looked at).  d_m and d_v may both be NULL: update_sumsq is 0; step, beta1, beta2, eps are ignored.
 * The work-item list of the table and the partial records live on the handle; a call whose table equals the one the handle holds uploads nothing.
 * A synchronous diagnostic call: it drains `stream` and fills h_out[n_tensors]; QPN_ESTATE while that stream is capturing.  It neither reads nor writes the status word,
 * the applied-update count or any other training state, and no launch of a training step differs for it.
 * Errors, checked before the device is looked at (also on a handle created without a GPU), QPN_EINVAL naming the argument: a NULL d_flat, h_tensor_end or h_out;
 * n_tensors < 1 or > 2^20; h_tensor_end[0] < 1, h_tensor_end not strictly ascending, or its last entry not n; only one of d_m / d_v; with moments step < 1, a beta outside
 * [0, 1), an eps that is NaN, infinite or negative.  A valid call without a GPU returns QPN_ENODEV. */
typedef struct qpn_tensor_stat {
    double grad_sumsq, weight_sumsq, update_sumsq;
    float grad_absmax, weight_absmax;
    int64_t grad_nonfinite;
} qpn_tensor_stat;
int qpn_tensor_stats(qpn_handle* h, const float* d_flat, const float* d_grad, const float* d_m, const float* d_v,
                     int64_t n, int step, float beta1, float beta2, float eps, const float* d_grad_denominator,
                     int n_tensors, const int64_t* h_tensor_end, qpn_tensor_stat* h_out, void* stream);

/* Per-launch-group device timings of the training calls issued between begin and end (HIP events on `stream`; used by bench.py for
 * the roofline).  h_ms[QPN_PG_*] receives milliseconds.  While a profile is being taken a step runs on ONE stream, and every heavy
 * kernel is a group of its own: LAYER_FWD / LAYER_BWD = the residual stack (one work-queue launch each at n_resch 64), WGRAD = the
 * gate contraction's weight gradient, WGRAD_WR / _SKIP / _POST / _CAUSAL = the residual 1x1's, the skip 1x1's, the post-net pair's and
 * the causal table's. */
#define QPN_PG_PREP 0
#define QPN_PG_LAYER_FWD 1
#define QPN_PG_POST_FWD 2
#define QPN_PG_CE 3
#define QPN_PG_POST_BWD 4
#define QPN_PG_WGRAD 5
#define QPN_PG_LAYER_BWD 6
#define QPN_PG_GRAD_TAIL 7
#define QPN_PG_ADAM 8
#define QPN_PG_ALLREDUCE 9     /* marked by the caller after its gradient all-reduce (qpn_train_profile_mark) */
#define QPN_PG_WGRAD_WR 10
#define QPN_PG_WGRAD_SKIP 11
#define QPN_PG_WGRAD_POST 12
#define QPN_PG_WGRAD_CAUSAL 13
#define QPN_PG_COUNT 14
/* Diagnostics of the one-launch residual stack (csrc/train_stack.hip; no reference counterpart): the first n <= 1024 control words of
 * the work queues as the last step left them -- [1] abort raised; forward [4..6] / backward [8..10]: escalations (a workgroup published
 * everything it held before waiting without a bound), polls spent waiting, waves that did not find their producers' flags at first look.  Synchronises the stream. */
int qpn_train_stack_stats(qpn_handle* h, unsigned* h_out, int n, void* stream);
/* Data-parallel step, two buckets (no reference counterpart: its DataParallel wrap, src/bin/qpnet_train.py:416-423, never runs with more than one
 * GPU).  After qpn_train_backward_ex(append_scale = 1) has been enqueued: [*first, *first + *count) is the tail of the exchange buffer -- the
 * post-net gradient blocks and the 4-float row-count trailer -- which the side stream completes while the layer backward is still running, and
 * `stream` is made to wait for exactly that (an event, no host wait).  The caller all-reduces that range on `stream`, the rest [0, *first) on
 * the stream the backward was enqueued on, and joins the two before qpn_adam_step_ex.  *count = 0: nothing finished early, exchange the whole buffer. */
int qpn_train_early_bucket(qpn_handle* h, int64_t* first, int64_t* count, void* stream);
/* First element of that tail (a property of the parameter layout; -1 if the layout has no such tail or the handle has not trained yet): ranks
 * agree on it ONCE before they split the exchange, so that every rank issues the same collectives in every step. */
int64_t qpn_train_early_first(qpn_handle* h);
int qpn_train_profile_begin(qpn_handle* h, void* stream);
/* The same with the step left as the timed loop runs it (the skip / post-net weight gradients, the early slab reduction, the aux tail and dWr on the
 * handle's side stream next to the stack backward and dW1): every launch is timed on the stream it runs on -- what a kernel costs INSIDE the
 * overlapped step (bench.py: roofline.overlapped, and the kernel the headline fraction is quoted for). */
int qpn_train_profile_begin_overlapped(qpn_handle* h, void* stream);
int qpn_train_profile_mark(qpn_handle* h, int group, void* stream);   /* attribute the work enqueued since the previous mark to `group` */
int qpn_train_profile_end(qpn_handle* h, float* h_ms, int n, void* stream);

/* _dilated_index (src/nets/qpnet.py:592-604, tensor path) and _generate_dilated_index
 * (src/nets/qpnet.py:613-618): d (B x L) float32 -> int64 (B x L), NOT replicated over
 * channels (the reference's .repeat over n_ch is redundant). */
/* The draw of sampling decode on logits the caller provides: row r of the row-major (n_rows x Q) fp32 matrix d_logits is drawn with the
 * Philox counter (step0 + r, row) and key `seed` -- what a decode call with that seed picks at step step0 + r of batch row `row` when
 * these are its logits there -- into d_out[r].  One wave per row runs the device function the decode kernels' picks run (the default
 * draw for (1.0f, 0), the controlled one otherwise).  Q in {64,128,...,1024} (a multiple of 64) as for sampling decode; temperature / top_k as for
 * qpn_decode_sampling, checked (like every argument: n_rows >= 1, row >= 0, step0 >= 0, step0 + n_rows <= 2^31) before a device is
 * looked for.  For sampling from teacher-forced logits (qpn_train_forward, the logits output of qpn_decode).  Asynchronous on `stream`. */
int qpn_sample_logits(const float* d_logits, int64_t n_rows, int Q, uint64_t seed, int row, int64_t step0, float temperature, int top_k,
                      int64_t* d_out, void* stream);
/* ... with top_p / min_p as for qpn_decode_sampling_ex, checked in the same place; qpn_sample_logits is this call with (1.0f, 0.0f). */
int qpn_sample_logits_ex(const float* d_logits, int64_t n_rows, int Q, uint64_t seed, int row, int64_t step0, float temperature, int top_k,
                         float top_p, float min_p, int64_t* d_out, void* stream);

/* Teacher-forced scoring of logits the caller provides (the per-sample view of what reference src/bin/qpnet_validate.py:409-437 averages into one
 * float per checkpoint): for every row of the (B x BL x Q) fp32 tensor d_logits and its target -- the LAST BL columns of the (B x tgt_stride) int64
 * tensor d_targets, as in qpn_ce_loss -- one 16-byte record in d_out[B * BL]:
 *   nll      lse - l[t] in nats, in the per-row arithmetic of qpn_ce_loss for that Q: the float64 sum of a chunk's nll over its row count IS that loss
 *   entropy  -sum p log p in nats, a class with p == 0 contributing 0 (finite for rows that hold -inf logits)
 *   argmax   the lowest index among the maxima (the decode kernels' rule)
 *   rank     #{q : l[q] > l[t]}, strict, on the raw floats: top-k accuracy is rank < k
 * A target outside [0, Q) gives nll = +inf and rank = Q (argmax and entropy stay valid): there is no handle, hence no status word.  A row with a NaN
 * logit, or with every logit -inf, is unspecified.  One wave per row; a row of Q <= 1024 is read from memory once.  Arguments are checked before a
 * device is looked for: QPN_EINVAL, naming the argument, for a NULL pointer, B < 1, BL < 1, Q outside 1..65536, tgt_stride < BL, B * BL >= 2^31.
 * For scoring teacher-forced logits (qpn_train_forward, the logits output of qpn_decode).  Asynchronous on `stream`. */
typedef struct { float nll; float entropy; int32_t argmax; int32_t rank; } qpn_score_row;
int qpn_score_logits(const float* d_logits, const int64_t* d_targets, int64_t tgt_stride, int B, int BL, int Q, qpn_score_row* d_out, void* stream);

/* Cut one training batch out of a device-resident corpus (what the reference's generator, src/bin/qpnet_train.py:200-335, assembles on the host for
 * every step; the reference has no device counterpart).  The corpus is three arenas, utterances back to back: d_samples, int16 mu-law class indices
 * [n_samples]; d_feats, fp32 scaled features [n_frames][n_aux] row-major; d_factors, fp32 dilated factors [n_frames], one per frame.  Row b of the batch is
 * the concatenation of the segments row_first[b] .. row_first[b + 1] - 1 of the table (row_first[0] = 0, row_first[B] = n_segs): n_samples samples from
 * sample0, n_frames feature rows from frame0, and for its samples the factors of the frames from factor0 on (sample s of the segment takes factor0 + s / U).
 * A segment may hold samples and no feature row.  A row's segments together hold T + 1 = frames * U + 1 samples and exactly `frames` feature rows.  Outputs,
 * every element written exactly once by ONE launch on `stream`, no host synchronisation:
 *   d_x int64 (B x T)               the row's samples [0, T)
 *   d_t int64 (B x T)               the row's samples [1, T + 1)
 *   d_h fp32  (B x n_aux x frames)  the row's feature rows, transposed
 *   d_d fp32  (B x T)               sample s gets the factor of the row's frame s / U
 *   d_w fp32  (B x bl), or NULL     1 where feature column 0 of the frame at position p / U is above 0.5, else unvoiced_weight; p runs over the last bl of
 *                                   the row's T positions
 * d_x, d_t, d_d and d_w must be 16-byte aligned.  The table is given twice: h_segs / h_row_first on the host, checked here before anything is launched, and
 * d_segs / d_row_first, a device copy of the same bytes that the caller has enqueued on `stream` and that the kernel reads.  A table that fails the check
 * returns QPN_ERANGE (a segment leaves an arena) or QPN_EINVAL (a negative count, a row whose sums are not T + 1 samples and `frames` rows, row_first not
 * monotone, U < 1, n_aux < 1, bl outside 1..T) with a message that names the row and the segment; nothing is launched then, so the kernel is never handed an
 * index outside the arenas and there is no status word.  No handle.  Arguments are checked before a device is looked for. */
typedef struct { int64_t sample0; int64_t frame0; int64_t factor0; int32_t n_samples; int32_t n_frames; } qpn_corpus_seg;
int qpn_cut_chunks(const int16_t* d_samples, int64_t n_samples, const float* d_feats, const float* d_factors, int64_t n_frames, int n_aux,
                   const qpn_corpus_seg* h_segs, const int32_t* h_row_first, const qpn_corpus_seg* d_segs, const int32_t* d_row_first, int64_t n_segs,
                   int B, int frames, int U, int bl, float unvoiced_weight,
                   int64_t* d_x, int64_t* d_t, float* d_h, float* d_d, float* d_w, void* stream);

int qpn_dilated_index_train(const float* d_d, int B, int64_t L, int dilation, int64_t* d_out, void* stream);
int qpn_dilated_index_gen_f32(const float* d_d, int64_t n, int dilation, int64_t* d_out, void* stream);
int qpn_dilated_index_gen_f64(const double* d_d, int64_t n, int dilation, int32_t* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QPNET_HIP_H */
