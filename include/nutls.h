/*
 * nutls.h -- C ABI of the MI355X-native NUNet-TLS frame-by-frame forward pass.
 *
 * This is the drop-in boundary for ONE path of the reference: the per-frame model call
 *
 *     runner = interpreter.get_signature_runner('nutls_lstm_sm')          (interpreter_proposed.py:380)
 *     out    = runner(input=..., msfe6_ee_prev1=..., ..., msfe6_de_c=...)  (interpreter_proposed.py:215-350)
 *
 * (phone twin: Interpreter.runSignature(inputs, outputs, "nutls_lstm_sm"),
 *  mobile_app/.../RTSE_NUTLS_LSTM.java:571), i.e. the function
 * TFL_SIGNITURE.nutls_lstm of converter_proposed.py:188-867 evaluated by TF-Lite.
 *
 * Differences from the reference surface, by design:
 *   - B independent streams per handle (the reference is batch 1);
 *   - the 130 recurrent-state tensors (converter_proposed.py:27-186) stay resident in HBM
 *     between calls; the caller may read / write any of them by its signature name
 *     (the "cur -> prev" echo of interpreter_proposed.py:215-350 becomes a buffer flip);
 *   - weights come from a .nutlsw container (tools/convert_tflite_weights.py), not a .tflite.
 *
 * Plain pointers and sizes only.  Every entry returns 0 on success or a negative code;
 * nutls_last_error() returns a thread-local message for the last failure.
 * One handle = one GPU = one host thread at a time (like a TF-Lite Interpreter).
 * Stream order: calls on one handle take effect in the order they are made, whichever streams they name, the _host entries' private
 * stream included.  A stream named in a call must outlive the handle's next call.  (nutls_step(h, ..., side) followed at once by
 * nutls_step_host(h, ...), by a step on another stream or by one with stream = NULL needs no synchronisation in between: a call that names
 * another stream than the call before it first waits, on the device, for an event recorded on that call's stream -- which is why that
 * stream must still exist.  Calls that stay on one stream pay a pointer compare.  What the CALLER queues on its streams -- the copies that
 * fill mag_in, the kernels that read mag_out -- is ordered by the caller, on the stream it hands over.)
 */
#ifndef NUTLS_H_
#define NUTLS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nutls_handle nutls_handle;

enum {
  NUTLS_OK = 0,
  NUTLS_ERR_ARG = -1,      /* bad argument: unknown state name, size mismatch, null pointer (ValueError in TF-Lite) */
  NUTLS_ERR_WEIGHTS = -2,  /* malformed weight container or missing tensor */
  NUTLS_ERR_HIP = -3,      /* HIP runtime failure (message carries hipGetErrorString) */
  NUTLS_ERR_NO_DEVICE = -4 /* no usable gfx950 device: there is NO CPU fallback */
};

enum {
  NUTLS_VARIANT_LSTM = 0,     /* NUNet-TLS-LSTM, "proposed" (models/proposed.py; signature 'nutls_lstm_sm', 130 states) */
  NUTLS_VARIANT_BASELINE = 1  /* NUNet-TLS with the dilated-dense bottleneck (models/nunet_tls.py; signature 'nutls'
                               * of converter_nunet_tls.py:1542, 208 states).  No trained weights exist for it. */
};

#define NUTLS_BINS 256        /* network bins per frame (DC dropped, interpreter_proposed.py:212-213) */
#define NUTLS_LSTM_UNITS 21   /* models/proposed.py:21 */

/* Replaces: tf.lite.Interpreter(model_path) + allocate_tensors() (interpreter_proposed.py:374-375).
 * `weights`/`n_bytes`: the .nutlsw container bytes (copied; caller may free after return).
 * `batch`: number of independent streams B (>= 1).  `device`: HIP device ordinal. */
int nutls_create(const void* weights, size_t n_bytes, int variant, int batch, int device,
                 nutls_handle** out);

/* nutls_create with the fused kernel's plan chosen by the caller: streams_per_workgroup = 0 (the library's choice, = nutls_create), 1, 2 or
 * 4 (see nutls_streams_per_workgroup).  An explicit count the batch is not a multiple of, or one the variant has no plan for (3, 8, ...;
 * the baseline variant has the one-stream plan only) is NUTLS_ERR_ARG; an explicit count (1, 2, 4) with a container the fused kernel
 * cannot run -- conv kernels not stored as int8 -- is NUTLS_ERR_WEIGHTS with the reason in nutls_last_error (nutls_create would run such a
 * container on the per-layer kernels, mode 1).  An explicit request never silently becomes another plan or another kernel family. */
int nutls_create_plan(const void* weights, size_t n_bytes, int variant, int batch, int device, int streams_per_workgroup,
                      nutls_handle** out);

/* Replaces: del interpreter. */
int nutls_destroy(nutls_handle* h);

/* Replaces: one runner(...) call for all B streams (interpreter_proposed.py:215-350) with the
 * cur->prev echo folded in.  mag_in / mag_out: DEVICE pointers to [B, 256] float32
 * (row = stream; bins 1..256 of |STFT|).  Asynchronous on `stream` (a hipStream_t, may be NULL
 * for the default stream); state advances by one frame.  In the fused mode the kernel reads mag_in and writes mag_out
 * directly (no staging copy): both must stay valid, and mag_in unmodified, until the work queued on `stream` has run;
 * they may be the same buffer.  Side effect that differs by mode: modes 0-2 compute on the library's own [B,256] buffers
 * (nutls_io_buffers) and copy to / from the caller's, so those library buffers hold the frame afterwards; the fused mode
 * writes ONLY the mag_out it was given.  Whatever reads the library's mag_out buffer after a step (nutls_istft_hop) therefore
 * needs the step to have run on the library buffers (pass the pointers of nutls_io_buffers, which is what nutls_enhance_hop
 * does) -- after nutls_step(h, user_in, user_out) in the fused mode that buffer still holds the frame of the last step that
 * was given it. */
int nutls_step(nutls_handle* h, const float* mag_in, float* mag_out, void* stream);

/* Same with HOST buffers: H2D copy, step, D2H copy, synchronises before returning.  With pageable memory (malloc, numpy) the two copies go
 * through the runtime's staging buffers; with buffers from nutls_host_alloc they are plain DMA transfers, and in the fused mode there are no
 * copies at all: the kernel reads the frame from and writes the result to the pinned host buffers over the link (PCIe) itself. */
int nutls_step_host(nutls_handle* h, const float* mag_in, float* mag_out);

/* ---- Per-stream active mask: step a chosen subset of the handle's streams ------------------------------------
 * The B streams of a handle are independent, and so is their time: a server that multiplexes calls onto one handle has slots whose
 * frame has not arrived at a tick (clock drift, jitter, a call that has not joined yet).  `active` is [B] bytes, one per stream:
 * nonzero = the stream takes this frame, zero = the stream is HELD.  A held stream, in one call:
 *   - keeps everything of it that survives the call exactly as it was: the 130 signature states as every accessor shows them, the
 *     carried partial sums of the two-tap convs, and (nutls_enhance_hop_active) its previous hop and overlap tail;
 *   - its row of mag_in / pcm_in has no effect (it may hold anything, NaN included).  It is not even read where the stream's whole
 *     workgroup is held -- always on the one-stream plan; on a packed plan a workgroup with held AND active slots runs the step for all
 *     of them, so the row is read and computed on there, and the results are then replaced by the held state and the zero row;
 *   - its row of mag_out / pcm_out is written with ZEROS (deterministic: never stale data, never the input).  (The _pcm entries of a handle
 *     in a G.711 format write the format's SILENCE code, 0xFF or 0xD5, in place of zero bytes: "PCM gateway", G.711.)
 * A stream that takes frames x0, x1, x2 at ticks 0, 3 and 4 produces the same bits -- outputs and states -- as one that took them at
 * ticks 0, 1 and 2; a held tick costs it nothing but time.  The other streams are not affected in any bit.  A new call joins a slot with
 * nutls_reset(h, b).  (The handle-wide state parity still flips on every call: a held stream's state is copied across, which is
 * why holding is not free -- about 1.9 MB of device traffic per held stream and call -- but it needs no weights and no arithmetic.)
 *
 * nutls_step_active / nutls_enhance_hop_active: `active` is a DEVICE pointer, read by the kernels: it must stay valid and unmodified
 * until the work queued on `stream` has run.  The _host entries take `active` in HOST memory (pageable or pinned) and copy the B bytes
 * themselves; with buffers from nutls_host_alloc nutls_step_host_active still runs without copies of the frames.
 * active == NULL means all streams: the call IS the entry without the mask (same code path, same bits).
 *
 * After nutls_state_set the masked launches write all 130 states of the active streams themselves (normally 40 conv-input states are left
 * to be rebuilt on demand, see nutls_state_get) until every stream has taken a frame since the edit -- the _host entries see the masks and
 * follow that; with DEVICE masks the library cannot, and the more expensive launches last until one call steps all streams (NULL mask).
 *
 * Supported: streaming handles of the LSTM variant in the fused mode (mode 3) with NUTLS_CTFA_FRAME, on every plan (1, 2 or 4 streams
 * per workgroup).  With a non-NULL mask everything else returns NUTLS_ERR_ARG (reason in nutls_last_error) and changes nothing -- never
 * a silent step of all streams:
 *   - modes 0 / 1: the per-layer plans and the captured graphs are handle-wide;
 *   - the baseline variant: its dilated-dense history rings are updated in place, at a slot derived from the handle's frame counter
 *     -- holding a stream there needs a ring position per stream;
 *   - NUTLS_CTFA_CAUSAL32 on a streaming handle: the same, for the time-attention ring;
 *   - offline handles (they step blocks of frames of one utterance each: nutls_process_block). */
int nutls_step_active(nutls_handle* h, const float* mag_in, float* mag_out, const unsigned char* active, void* stream);
int nutls_step_host_active(nutls_handle* h, const float* mag_in, float* mag_out, const unsigned char* active);

/* Page-locked, device-visible host memory for the buffers handed to nutls_step_host / nutls_enhance_hop_host / nutls_process_block_host
 * (what TF-Lite's interpreter.tensor(i) zero-copy view is to set_tensor / get_tensor in the reference's loop, interpreter_proposed.py:215-350:
 * the caller produces its frames in, and consumes its results from, memory the device can reach).  NULL on failure (nutls_last_error).
 * A handle is not needed; the memory is visible to every device.  A buffer counts as page-locked when all of it lies inside ONE such
 * allocation (any offset); one that starts inside an allocation and runs past its end takes the staged copies of pageable memory. */
void* nutls_host_alloc(size_t bytes);
void nutls_host_free(void* p);

/* ---- STFT front end / inverse-STFT back end on the device -----------------
 * Replaces the numpy part of the reference's real_time_speech_enhancer loop
 * (dnn_model/interpreter_proposed.py:203-213 analysis, :352-365 synthesis): frame 512, hop 256,
 * analysis window = periodic Hann with end taps 1e-7 (:20-22), inverse window (:24-26), overlap-add.
 * The library keeps, per stream, the previous hop and the overlap tail (zeroed by nutls_reset).
 *
 * nutls_enhance_hop: pcm_in / pcm_out are DEVICE pointers to [B, 256] float32 (row = stream, one hop of
 * 256 samples): analysis -> model step -> synthesis, asynchronous on `stream`.  Like the reference loop the
 * output lags the input by one hop (the first returned hop is the leading half-window).
 * dc_mode: how bin 0 is re-created behind the 256-bin model. */
#define NUTLS_DC_EDGE 0   /* PC loop: np.pad(..., mode='edge'), interpreter_proposed.py:352-353 */
#define NUTLS_DC_ZERO 1   /* phone: zero, mobile_app/.../RTSE_NUTLS_LSTM.java:677 */
int nutls_enhance_hop(nutls_handle* h, const float* pcm_in, float* pcm_out, int dc_mode, void* stream);
/* Same with HOST buffers (H2D, pipeline, D2H, synchronises). */
int nutls_enhance_hop_host(nutls_handle* h, const float* pcm_in, float* pcm_out, int dc_mode);
/* The same with a per-stream active mask (see nutls_step_active: `active` a DEVICE pointer here, HOST memory in the _host entry; NULL =
 * nutls_enhance_hop): analysis, model step and synthesis all skip the held streams -- previous hop, overlap tail and model state stay
 * as they are, the held rows of pcm_out are zero hops.  Each stream's concatenated active hops equal what a handle fed in lockstep returns. */
int nutls_enhance_hop_active(nutls_handle* h, const float* pcm_in, float* pcm_out, const unsigned char* active, int dc_mode, void* stream);
int nutls_enhance_hop_host_active(nutls_handle* h, const float* pcm_in, float* pcm_out, const unsigned char* active, int dc_mode);
/* The two halves on their own (testing, custom models): analysis of one hop into the library's mag_in buffer
 * (+ phase kept inside), synthesis of one hop from the library's mag_out buffer.  Device pointers.
 * nutls_istft_hop honours the attenuation limit ("Attenuation limit" below): while a row's limit is not 0 it also reads the library's
 * mag_in buffer, as the last nutls_stft_hop left it, as the noisy rows of the frame. */
int nutls_stft_hop(nutls_handle* h, const float* pcm_in, void* stream);
int nutls_istft_hop(nutls_handle* h, float* pcm_out, int dc_mode, void* stream);

/* ---- Hop fusion: the streaming hop as ONE launch --------------------------------------------------------------
 * By default nutls_enhance_hop is three launches -- analysis, model step, synthesis -- and the 256 magnitudes and 257 phasors of every
 * stream go through device memory between them.  With hop fusion on, the four nutls_enhance_hop* entries issue one launch of a hop build of
 * the fused step kernel: one wavefront per stream transforms the new hop in front of the first layer (a 256-point complex transform on the
 * real frame, in registers and the wave's own shared memory), one transforms the estimate back and overlap-adds behind the last layer.
 *   - Same state, same buffers: previous hop, overlap tail, phasors and the library's mag_in / mag_out rows (nutls_io_buffers) keep their
 *     layouts and meanings, so fusion may be switched between any two hops of a live stream, nutls_reset works as before, and
 *     nutls_debug_get("phasor") / the io buffers show the same things.  The transform is the waveform block mode's (nutls_stft_block), not
 *     the three-launch path's radix-2 one: outputs agree with the three-launch path to rounding (1e-5 relative RMS), not bit for bit.
 *   - Masks: nutls_enhance_hop_active behaves as documented above -- held rows of pcm_out are zero hops, a held stream's previous hop,
 *     overlap tail and phasors stay, its pcm_in row is not read where its whole workgroup is held.
 *   - Host buffers: when BOTH buffers of nutls_enhance_hop_host(_active) come from nutls_host_alloc the kernel reads and writes them over
 *     the link itself (no copy commands); pageable buffers keep the staged copies.
 *   - Unchanged: nutls_stft_hop, nutls_istft_hop, nutls_step* and every call on a handle with fusion off run the kernels they always ran.
 * Default: off.  NUTLS_HOP_FUSION=1 in the environment at creation turns it on for handles that support it (quietly off elsewhere).
 *
 * Supported: streaming handles of the LSTM variant in the fused mode (mode 3) on the one- and two-stream plans, either CTFA mode.
 * nutls_set_hop_fusion(h, nonzero) returns NUTLS_ERR_ARG (reason in nutls_last_error) and changes nothing on: the baseline variant, the
 * four-stream plan, modes 0 / 1, offline handles, a handle with nutls_debug_trace on.  While fusion is on, nutls_debug_trace(h, 1),
 * nutls_set_mode(h, 0 or 1), nutls_use_graph and the nutls_profile_* entries are refused the same way: an explicit request for one
 * launch per hop never silently becomes three.  nutls_set_hop_fusion(h, 0) always succeeds.
 * nutls_launches_per_hop: 3, or 1 with fusion on. */
int nutls_set_hop_fusion(nutls_handle* h, int enable);
int nutls_launches_per_hop(nutls_handle* h);
/* Waveform block mode: the same front end / back end for OFFLINE handles (nutls_create_offline, nutls_create_offline_batch; a streaming
 * handle gets NUTLS_ERR_ARG), a whole block per call -- the loop of interpreter_proposed.py:203-213, 352-365 over n_hops hops of every
 * utterance in one analysis launch and one synthesis launch around nutls_process_block.
 * pcm_in / pcm_out: DEVICE [utterances, n_hops * 256] float32 (8-byte aligned), 1 <= n_hops <= max_frames.  Analysis of n_hops hops of
 * every utterance -> nutls_process_block on the library's buffers -> synthesis; asynchronous on `stream`.  Like nutls_enhance_hop the
 * output lags the input by one hop.  Previous hop and overlap tail are carried per utterance from call to call, so a recording may be
 * cut into blocks of any lengths (the result does not depend on the cut); nutls_reset(h, u) zeroes utterance u's (-1: everybody's). */
int nutls_enhance_block(nutls_handle* h, const float* pcm_in, float* pcm_out, int n_hops, int dc_mode, void* stream);
/* Same with HOST buffers (pageable or nutls_host_alloc); synchronises. */
int nutls_enhance_block_host(nutls_handle* h, const float* pcm_in, float* pcm_out, int n_hops, int dc_mode);
/* The two halves on their own.  mag: DEVICE [utterances, n_hops, 256] (bins 1..256, the layout nutls_process_block takes); the phasors stay
 * inside the handle, so the synthesis belongs to the last analysed block and takes the same n_hops. */
int nutls_stft_block(nutls_handle* h, const float* pcm_in, float* mag, int n_hops, void* stream);
int nutls_istft_block(nutls_handle* h, const float* mag, float* pcm_out, int n_hops, int dc_mode, void* stream);

/* ---- Offline / block mode ------------------------------------------------
 * One utterance, up to `max_frames` consecutive frames per call: the frame index takes the place of the stream
 * index (a conv layer's previous-frame tap is the same tensor one frame earlier), every conv-like layer runs once
 * per block over all frames, only the 13 LSTM recurrences are scanned sequentially.  Same function as feeding the
 * frames one by one to a batch-1 streaming handle (the offline formulation of models/proposed.py:284-625 with the
 * streaming CTFA of converter_proposed.py:258-262); the state carries over from block to block inside the handle
 * and is zeroed by nutls_reset(h, -1).  mag_in / mag_out: DEVICE pointers to [n_frames, 256] float32. */
int nutls_create_offline(const void* weights, size_t n_bytes, int max_frames, int device, nutls_handle** out);
/* The same with a BATCH dimension -- the offline forward of the reference takes [B, T, ...] (models/proposed.py:284-625): `utterances`
 * (1 .. 256, utterances x max_frames <= 65536) independent utterances per handle, every call processes the same number of frames of each:
 * mag_in / mag_out are [utterances, n_frames, 256].  Every conv-like layer is ONE launch over the frames of all utterances, the 13 LSTM
 * recurrences of the utterances are scanned side by side (one wavefront each).  Each utterance carries its own state from block to block;
 * nutls_reset(h, u) zeroes utterance u (-1: all), nutls_state_get / _set take [utterances, ...] buffers, nutls_state_get_all(h, u, ...) one
 * utterance's.  Results per utterance equal those of a one-utterance handle (same kernels, same tilings). */
int nutls_create_offline_batch(const void* weights, size_t n_bytes, int max_frames, int utterances, int device, nutls_handle** out);
int nutls_process_block(nutls_handle* h, const float* mag_in, float* mag_out, int n_frames, void* stream);
/* The frequency-attention branch of CTFA in offline handles:
 *   NUTLS_CTFA_FRAME     (default) what the frame-wise graph computes: the branch sees TA/32 (ctfa_rt with T = 1,
 *                        proposed.py:162-196) -- offline results equal the streaming ones;
 *   NUTLS_CTFA_CAUSAL32  the offline / training model (`ctfa`, proposed.py:125-160, :143-147): the mean of the time
 *                        attention over the last 32 real frames (zeros before the utterance starts).  The 31-frame
 *                        history carries from block to block; switching modes or nutls_reset clears it. */
#define NUTLS_CTFA_FRAME 0
#define NUTLS_CTFA_CAUSAL32 1
int nutls_offline_set_ctfa_mode(nutls_handle* h, int mode);
/* The same choice for any handle.  Offline handles: as above.  Streaming handles (fused kernel, mode 3, only): NUTLS_CTFA_CAUSAL32 keeps
 * the time attention of the last 32 frames of every stream and stage in the library (not a signature tensor: the reference's streaming
 * graph has no such state) and feeds the frequency branch their mean -- streaming then equals the offline / training
 * model's attention (proposed.py:143-147) frame by frame.  nutls_reset clears a stream's history, a mode switch everyone's. */
int nutls_set_ctfa_mode(nutls_handle* h, int mode);
/* Block pipeline of an offline handle.  Only the 13 LSTM recurrences are serial over the frames of a block, and every
 * layer is causal in time, so a block is cut into `chunks` runs of consecutive frames: chunk 0 executes on the caller's
 * stream, chunk c > 0 on its own HIP stream one bottleneck behind chunk c-1 (it needs that chunk's last frame:
 * previous-frame taps, h / c, time-attention history), and the scans of one chunk overlap the convolutions of the others.
 * Results do not depend on the chunk count.  chunks: 1 .. 16, or 0 (default) = chosen from the block length (2 from 256
 * frames on, 3 from 768: the GPU serves four compute queues at a time, a pipeline with more queues than that
 * serialises -- 4 chunks need GPU_MAX_HW_QUEUES >= 8 and are no faster than 3). */
int nutls_offline_set_pipeline(nutls_handle* h, int chunks);
/* Same with HOST buffers (synchronises). */
int nutls_process_block_host(nutls_handle* h, const float* mag_in, float* mag_out, int n_frames);

/* ---- Ragged blocks: per-utterance frame counts for the offline batch handles ------------------------------------
 * nutls_process_block steps the same number of frames of every utterance; recordings never have equal lengths.  The entries below take,
 * beside the block's row stride n_frames / n_hops (1 .. max_frames), `frames` / `hops`: [utterances] int, frames[u] in 0 .. n_frames = how
 * many LEADING frames of utterance u are real.  Buffers keep their layouts, [utterances, n_frames, 256] and [utterances, n_hops * 256]
 * (with counts: 16-byte aligned).  For utterance u with k = frames[u], one call
 *   - writes rows 0 .. k-1 of mag_out / pcm_out with exactly the bits the uniform call of the same width on the same handle writes there
 *     (the model runs the same launches at the same sizes: every layer is causal in time and utterances never mix, so a frame does not
 *     depend on the rows behind it or on another utterance);
 *   - writes rows k .. n_frames-1 of the output with ZEROS.  The matching input rows have no effect on any result and may hold anything,
 *     NaN included: they are replaced by zeros on the way into the library's own input buffer (the waveform entries never read those PCM
 *     rows and write zero magnitudes).  The caller's input buffer is never written;
 *   - carries to the next call what belongs to frame k, not to frame n_frames: the 130 state tensors, under NUTLS_CTFA_CAUSAL32 the 31-row
 *     time-attention history of each of the 12 stages, in the waveform entries the previous hop (hop k-1) and the overlap tail (second
 *     half of frame k-1).  nutls_debug_get("phasor_block") rows >= k are unspecified;
 *   - k = 0 HOLDS the utterance: everything it carries stays exactly as it was.
 * An utterance that receives its frames in ragged calls of counts k1, k2, ... therefore produces the same concatenated result as any other
 * cut of the same frames on a handle of the same shape; a recording that ends frees its slot with nutls_reset(h, u), and the next one
 * joins the slot in the next block without disturbing the others.
 *
 * nutls_process_block_ragged / nutls_enhance_block_ragged / nutls_stft_block_ragged / nutls_istft_block_ragged: the counts are a DEVICE
 * pointer, read by the kernels: it must stay valid and unmodified until the work queued on `stream` has run.  The host cannot see those
 * counts (and does not synchronise to look): the kernels clamp them to 0 .. n_frames.  The _host entries take the counts in HOST memory,
 * check them -- one outside 0 .. n_frames is NUTLS_ERR_ARG, and nothing has been touched -- and copy them themselves.
 * frames == NULL / hops == NULL means every frame of every utterance: the call IS the entry without counts (same code path, same bits).
 *
 * Supported: offline handles (nutls_create_offline, nutls_create_offline_batch), both CTFA modes, every nutls_offline_set_pipeline chunk
 * count.  A streaming handle gets NUTLS_ERR_ARG from all six (its streams run on their own clocks with nutls_step_active).
 * Cost: a ragged block costs what the uniform block of its row stride costs -- the frames behind a count are computed and discarded;
 * skipping them inside the layers' launches is not attempted -- plus three small copy kernels: the masked copies in and out and the
 * per-utterance gather of the carried state (in place of the uniform call's two copies and its strided copy of the last slot; the gather
 * moves one arena slot per utterance).  Choose the row stride as the longest count of the block. */
int nutls_process_block_ragged(nutls_handle* h, const float* mag_in, float* mag_out, int n_frames, const int* frames, void* stream);
int nutls_process_block_ragged_host(nutls_handle* h, const float* mag_in, float* mag_out, int n_frames, const int* frames);
int nutls_enhance_block_ragged(nutls_handle* h, const float* pcm_in, float* pcm_out, int n_hops, const int* hops, int dc_mode, void* stream);
int nutls_enhance_block_ragged_host(nutls_handle* h, const float* pcm_in, float* pcm_out, int n_hops, const int* hops, int dc_mode);
/* The two halves on their own, as nutls_stft_block / nutls_istft_block: the synthesis belongs to the last analysed block (same n_hops; pass
 * the same counts). */
int nutls_stft_block_ragged(nutls_handle* h, const float* pcm_in, float* mag, int n_hops, const int* hops, void* stream);
int nutls_istft_block_ragged(nutls_handle* h, const float* mag, float* pcm_out, int n_hops, const int* hops, int dc_mode, void* stream);

/* ---- PCM gateway: the callers' sample rate and sample type, converted on the device -----------------------------------------
 * Every waveform entry above takes and returns float32 samples at exactly 16 kHz (the reference refuses anything else:
 * interpreter_proposed.py:384-385); telephony delivers 16-bit samples at 8 kHz, capture devices and WebRTC 48 kHz, the phone app 16-bit PCM
 * (AudioFormat.ENCODING_PCM_16BIT).  A handle is told its callers' format once; the _pcm entries below then take and return that audio and
 * keep the resampler state per stream, next to the state the library already owns.
 *
 * Format: rate_hz = 8000, 16000, 32000 or 48000; sample_format = NUTLS_PCM_F32 or NUTLS_PCM_S16 (at 8000 also NUTLS_PCM_ULAW or
 * NUTLS_PCM_ALAW, one byte per sample: "G.711" below).  A hop stays 16 ms at every rate:
 * S = 256 * rate / 16000 samples (128, 256, 512, 768).  Buffers are [B, S] (hops) / [utterances, n_hops * S] (blocks) of the sample type,
 * rows contiguous, base pointer 16-byte aligned.  A handle starts at 16000 / NUTLS_PCM_F32.  nutls_set_pcm_format may be called between any
 * two hops; it zeroes every stream's resampler history (as a mode switch starts a new history) and synchronises the device.  Another rate or
 * format is NUTLS_ERR_ARG and changes nothing.  The format applies to the _pcm entries ONLY: nutls_enhance_hop, nutls_enhance_block,
 * nutls_stft_hop / _block, nutls_istft_hop / _block and their variants keep taking float32 at 16 kHz, whatever was set.
 * At 16000 / NUTLS_PCM_F32 the _pcm entries ARE the plain entries: same code path, same bits, no extra launch, no delay.
 *
 * Samples: int16 -> float is s / 32768 (exact); float -> int16 is y * 32768 rounded to nearest even and clamped to -32768 .. 32767, NaN -> 0.
 * The float that is quantised is bit for bit the value the NUTLS_PCM_F32 format returns.
 *
 * G.711 (NUTLS_PCM_ULAW, NUTLS_PCM_ALAW; 8000 Hz ONLY): what telephony delivers on the wire -- RTP payload types 0 (PCMU) and 8 (PCMA), the
 * .wav / .au archives of call recordings -- is one BYTE per sample, mu-law or A-law.  Buffers are [B, 128] bytes for a hop and
 * [utterances, n_hops * 128] bytes for a block, rows contiguous, base pointer 16-byte aligned; nutls_pcm_hop_samples and
 * nutls_pcm_delay_samples are what they are at 8 kHz (128 and 48).  Either format at any other rate is NUTLS_ERR_ARG and changes nothing: an
 * explicit request never silently becomes another format.  Everything else about a format switch is as above.  The companding is a pure
 * bit rule, exact in both directions (the rules of the widely used g711.c and of CPython's audioop.ulaw2lin / alaw2lin / lin2ulaw / lin2alaw
 * at width 2), with c the byte and >> an arithmetic shift:
 *   expansion (decode): the code is mapped to an int16 value s, then s / 32768 exactly; from there on the chain is the int16 format's, so a
 *   companded handle fed codes c and an int16 handle fed expand(c) produce the same bits everywhere downstream.
 *     mu-law: u = ~c & 0xFF; t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4); s = (u & 0x80) ? 0x84 - t : t - 0x84.       Range +-32124.
 *     A-law:  a = c ^ 0x55; t = (a & 15) << 4; g = (a & 0x70) >> 4; t = g == 0 ? t + 8 : (t + 0x108) << (g - 1); s = (a & 0x80) ? t : -t.
 *             Range +-32256.
 *   compression (encode): the float is first quantised to int16 s exactly as NUTLS_PCM_S16 does it (y * 32768, round to nearest even, clamp,
 *   NaN -> 0: bit for bit the value the int16 format returns), then
 *     mu-law: v = s >> 2; if v < 0: v = -v, mask = 0x7F, else mask = 0xFF; v = min(v, 8159) + 33; seg = how many of the ends 0x3F, 0x7F, 0xFF,
 *             0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF v exceeds; code = (seg >= 8 ? 0x7F : (seg << 4) | ((v >> (seg + 1)) & 15)) ^ mask.
 *     A-law:  v = s >> 3; if v < 0: v = -v - 1, mask = 0x55, else mask = 0xD5; seg counted over 0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF,
 *             0xFFF; code = (seg >= 8 ? 0x7F : (seg << 4) | ((seg < 2 ? v >> 1 : v >> seg) & 15)) ^ mask.
 *   - mu-law never produces 0x7F: that code is negative zero, 0xFF is produced instead.  Every A-law code is a fixed point of expand ->
 *     compress, and so is every mu-law code except 0x7F.
 *   - SILENCE, NOT ZEROS: a zero byte is full-scale negative in mu-law and -5504 in A-law.  Wherever this header says that a row or hop of
 *     pcm_out is written with ZEROS -- a held stream under an `active` mask, the hops behind a ragged count -- a companded handle writes the
 *     format's silence code instead: 0xFF (mu-law) or 0xD5 (A-law), what compressing a zero hop gives; it expands to 0 and to +8.
 *   - nutls_pcm_g711_expand(fmt, table, 256) and nutls_pcm_g711_compress(fmt, in, out, n) are the library's statement of the rule, host only,
 *     no handle and no GPU, as nutls_pcm_filter is: the int16 value of each of the 256 codes, and the codes of n int16 values.  A format other
 *     than the two, a null pointer or a table length other than 256 is NUTLS_ERR_ARG, and nothing is written.  The kernels agree with them bit
 *     for bit.
 *   - Every _pcm entry at 8 kHz honours the two formats: the hop entries (nutls_enhance_hop_pcm, _active, _host, _host_active), the halves
 *     nutls_pcm_decode_hop / nutls_pcm_encode_hop, the block entries (nutls_enhance_block_pcm, _host, the _ragged forms) and the block halves
 *     with and without counts; hop fusion on or off, the attenuation limit, masks, nutls_reset and in-place pcm_in == pcm_out apply
 *     unchanged.  The upper band and follow are refused as on every 8 kHz handle.  The _host entries move a quarter of the float32 bytes.
 *
 * Rates: q = max(rate, 16000) / min(rate, 16000) = 2 or 3.  One linear-phase FIR prototype p[0 .. 2 K q] per rate, K = 24: a Kaiser-windowed
 * sinc (beta 8) with its cutoff at the LOWER rate's Nyquist frequency, designed in double when needed, normalised to sum 1 and rounded to
 * fp32 once -- nutls_pcm_filter returns exactly the numbers the kernels use (in units of that Nyquist frequency: within 0.01 dB up to 0.85,
 * -6 dB at 1.0, at least 80 dB down from 1.15; symmetric to the bit; 2 K q + 1 taps, the single tap 1.0 for 16000).  The conversion is plain
 * causal filtering of a stream's concatenated samples from a zero state (samples before the first are zeros):
 *   rate reduction by q:  y[m] = sum_j p[j] x[q m - j]                          (scipy: upfirdn(p, x, 1, q))
 *   rate increase by q:   zero-stuff by q, then filter with q p                 (scipy: upfirdn(q p, x, q, 1))
 * both truncated to the input's length times the ratio.  A rate above 16 kHz is reduced on the way in and increased on the way out, 8 kHz
 * the other way round.  Each direction delays by K samples of the lower rate: nutls_pcm_delay_samples = 2 K max(1, rate / 16000) samples at
 * the caller's rate for the two together (0 at 16000); the one-hop lag of nutls_enhance_hop stays on top of it.
 *
 * Upper band (32 and 48 kHz): the model runs at 16 kHz, so what it returns is band-limited to 8 kHz.  nutls_set_pcm_upper_band(h, gain), gain
 * in 0 .. 1, passes the band above 8 kHz AROUND the model: it waits beside it for exactly the model's latency and is added back at that gain.
 * With D the decode half, E the encode half, M the model path with its one-hop lag, q = rate / 16000 and S = 256 q, per stream
 *   u[n]   = x[n - 2 K q] - E(D(x))[n]        the input, delayed by nutls_pcm_delay_samples, minus its own low band
 *   out[n] = E(M(D(x)))[n] + gain * u[n - S]  (samples before a stream's first are zeros)
 * The delay and the alignment are those without it: one hop plus nutls_pcm_delay_samples.  With M the identity and gain 1 the output is the
 * delayed input, whatever the filter.  The crossover is the prototype's own, 1 - H^2: at most -76 dB up to 0.85 of 8 kHz (the noisy input's low
 * band does not leak back), -15 dB at 0.95, -2.5 dB at 8 kHz, 0 dB from 1.05.
 *   - gain 0, the default, is off: the _pcm entries are then exactly what they are without this call -- same kernels, same bits.
 *   - A gain that is NaN or outside 0 .. 1 is NUTLS_ERR_ARG and changes nothing.  So is a gain other than 0 on a handle whose rate is 8000 or
 *     16000: there is no band above 8 kHz there, and an explicit request never silently does nothing.
 *   - The call is allowed between any two hops.  Like a format switch it synchronises the device and zeroes every stream's resampler
 *     histories and upper-band state.  Setting the value the handle already has is a no-op that touches nothing.  nutls_pcm_upper_band reads
 *     the gain back.  nutls_set_pcm_format turns the upper band OFF (gain 0), because a new format starts anew: set the gain after the format.
 *   - Every _pcm entry honours the gain, in the two launches it already makes: hop, _active, _host, _host_active, block, block _host and the
 *     _ragged entries; hop fusion on or off makes no difference.  So do the halves: nutls_pcm_decode_hop / _block(_ragged) record u of what they
 *     decode, nutls_pcm_encode_hop / _block(_ragged) add gain * u that belongs to the handle's LAST DECODED hop or block -- the contract
 *     nutls_istft_block has with the last analysed block: same n_hops, same counts, same mask.  Their signatures are what they were.
 *   - State, per stream (utterance), outside the signature's tensors, allocated when a gain other than 0 is first set: the last 2 K decoded
 *     samples and the last hop of u.  It obeys the rules of the resampler history below (nutls_reset, held streams, blocks, ragged counts --
 *     a count k carries it from hop k - 1, k = 0 holds it --, refusals before the first conversion).
 *   - Operation order, fp32, the same sequence for every output sample wherever it lies in its hop or block and whichever entry runs it:
 *       d[m]   = the rate reduction's sum: taps ascending, one FMA each, from 0                                 (2 K q + 1 FMAs)
 *       c[n]   = the rate increase's sum over d: taps ascending, one FMA each, from 0, the zero-stuffed terms skipped, WITHOUT its product
 *                by q                                                                                           (at most 2 K + 1 FMAs)
 *       u[n]   = fma(-q, c[n], x[n - 2 K q])                                                                    (one FMA)
 *       z[n]   = the output sample without the upper band (the rate increase's sum over the model's output, then its product by q)
 *       out[n] = fma(gain, u[n - S], z[n])                                                                      (one FMA)
 *     The longest path of an output sample has N = 2 K q + 2 K + 4 roundings; its error is at most (N + 3) 2^-24 times
 *     q sum |p| |M(D(x))| + gain (|x[n - 2 K q - S]| + q sum |p| (sum |p| |x|)), the absolute products along those sums.
 *     int16 output is that float, rounded to nearest even and saturated: bit for bit what NUTLS_PCM_F32 returns, then quantised.
 *   - In place: the _pcm device entries read pcm_in in their decode launch only, which has run before the encode launch writes pcm_out, so
 *     pcm_in == pcm_out (the same base pointer; no other overlap) is allowed, with the upper band on as with it off: u waits in a library buffer.
 *   - Cost: README, "PCM gateway".
 *   - Follow (nutls_set_pcm_upper_follow(h, 1)): the gain of nutls_set_pcm_upper_band becomes the CEILING of a gain that follows the suppression
 *     the model applied below 8 kHz, the "follow" mode of band-split suppressors: in a pause the hiss above 8 kHz goes where the noise below it
 *     went, in speech the upper band comes back at the ceiling.  Hops are counted per row (a stream or an utterance): t runs over the row's real
 *     hops since its last reset or format, gain or follow switch; hops before the first have energy 0; held ticks and hops behind a ragged count
 *     do not exist for this count.  d_t = the 256 decoded 16 kHz samples of hop t (what the decode half writes); y_t = the 256 samples the encode
 *     half is handed for hop t (in the _pcm entries the model's output, which lags d by one hop).  All arithmetic is fp32, every operation
 *     rounded on its own (no contraction; / and sqrt correctly rounded), in this one order:
 *       E2(v)  : s[i] = v[i] * v[i]; for h = 128, 64, ..., 1: s[i] = s[i] + s[i + h], i < h; the result is s[0]
 *       a_t = E2(d_t)            b_t = E2(y_t)
 *       A_t = ((a_{t-1} + a_{t-2}) + a_{t-3}) + a_{t-4}      W = NUTLS_PCM_FOLLOW_HOPS = 4 hops; shifted by the model's one-hop lag
 *       B_t = ((b_t + b_{t-1}) + b_{t-2}) + b_{t-3}
 *       g_t = gain * fminf(sqrt(B_t / fmaxf(A_t, 0x1p-100f)), 1)
 *       delta_t = g_t - g_{t-1};  w[n] = float(n + 1) * float32(1.0 / S);  gamma_t[n] = fmaf(delta_t, w[n], g_{t-1})     n = 0 .. S - 1
 *       out[n] = fmaf(gamma_t[n], u[n - S], z[n])                                         in place of fmaf(gain, u[n - S], z[n]) above
 *     gamma is a linear ramp across the hop that ends at g_t (w[S - 1] is exactly 1 for S = 512 and 768): no step at a hop edge.  g_{t-1} is
 *     the same formula on the windows one hop earlier, not a recurrence: every g is a function of at most 5 values of a and 5 of b, so every
 *     output sample is the same sequence of operations wherever a hop, block or tick boundary falls, and a and b are the same bits on the same
 *     samples (one energy code for both halves).  Where y_t = c d_{t-1} with c a power of two, g_t = gain * min(c, 1) exactly, and from the
 *     second such hop on out is bit for bit the fixed gain's.  Errors, to first order: A_t and B_t carry 12 roundings on non-negative terms,
 *     |g32 - g| <= 20 * 2^-24 g, |gamma32 - gamma| <= 24 * 2^-24 gain, and out is within the bound above taken at the ceiling plus
 *     24 * 2^-24 gain (|x[n - 2 K q - S]| + q sum |p| (sum |p| |x|)).
 *       . Enabling follow while the gain is 0 is NUTLS_ERR_ARG and changes nothing -- that is every 8000 / 16000 Hz handle.  Setting the value the
 *         handle already has is a no-op that touches nothing.  A real change synchronises and zeroes every row's resampler histories,
 *         upper-band and follow state, as a gain change does.  nutls_set_pcm_upper_band(h, 0) and nutls_set_pcm_format turn follow OFF; a
 *         change from one gain other than 0 to another keeps it (and zeroes the state, as ever).  nutls_pcm_upper_follow reads it back.
 *       . Follow off, every entry launches exactly the kernels it launches without this call -- same bits.  On, every _pcm entry honours it in the
 *         two launches it already makes: hop, _active, _host, _host_active, block, block _host, the _ragged entries; hop fusion on or off makes
 *         no difference.  So do the halves, signatures unchanged: the decode half records a of what it decodes, the encode half uses the a of the
 *         handle's LAST DECODED hop or block -- the contract it has for u.
 *       . State per row, allocated when follow is first enabled: the last 5 a, the last 4 b and the last g.  It obeys the rules of the last hop
 *         of u: nutls_reset zeroes it, a held row's is not touched, a count k carries it from hop k - 1, k = 0 holds it.
 *       . nutls_pcm_follow_gain(h, gains, n): HOST gains[rows] = g of each row's last real encoded hop (0 after a reset); synchronises the
 *         device.  NUTLS_ERR_ARG with follow off or n other than the handle's rows (streams / utterances).
 *
 * State: per stream (utterance) and direction the library keeps the filter's last 2 K q input samples, outside the signature's tensors.
 * nutls_reset(h, b) zeroes stream b's (-1: everybody's).  A held stream (active[b] == 0) keeps it as it is -- neither kernel touches it -- and
 * its row of pcm_out is zeros (G.711: the silence code, 0xFF / 0xD5, not zero bytes); its row of pcm_in is not read.  An offline handle carries it from block to block.  Every output sample is the
 * same sum, in the same order (taps ascending, one fp32 FMA each; the zero-stuffed terms skipped), over the same values wherever the hop or
 * block boundary falls: the two halves are bit-exact across every cut of a stream, between ticks 0, 3, 4 and ticks 0, 1, 2, and between the
 * hop entries of a streaming handle and the block entries of an offline one.
 *
 * Where: the hop entries wherever nutls_enhance_hop works (both variants, every mode, hop fusion on or off); the masked ones wherever
 * nutls_enhance_hop_active works, with the same refusals (checked before anything is converted: a refused call changes nothing).  Each
 * _pcm entry decodes into a library buffer, calls that plain entry on library buffers and encodes: two small launches more per hop or block.
 * An offline handle gets NUTLS_ERR_ARG from the hop entries, a streaming handle from the block entries.
 * The _host entries copy the raw samples (pageable or nutls_host_alloc) into library buffers, run the pipeline and copy back; they
 * synchronise like their float twins -- int16 moves half the bytes over the link, G.711 a quarter.  nutls_enhance_hop_pcm_host_active hands its mask on as
 * a device mask (see nutls_step_active on nutls_state_set and masks the host has not seen).  Ragged blocks in the callers' format: the
 * _pcm_ragged entries at the end of this section.  Zero-copy reads of pinned PCM stay out of scope: the _host entries copy. */
#define NUTLS_PCM_F32 0   /* float32, unit scale (what nutls_enhance_hop takes) */
#define NUTLS_PCM_S16 1   /* int16, little endian; 32768 = 1.0 */
#define NUTLS_PCM_ULAW 2  /* G.711 mu-law, one byte per sample (RTP PCMU); 8000 Hz only */
#define NUTLS_PCM_ALAW 3  /* G.711 A-law, one byte per sample (RTP PCMA); 8000 Hz only */
int nutls_set_pcm_format(nutls_handle* h, int rate_hz, int sample_format);   /* also turns the upper band off (gain 0), and follow with it */
/* G.711 above, host only, no handle: table[256] = the int16 value of every code; out[n] = the codes of in[n].  sample_format: NUTLS_PCM_ULAW
 * or NUTLS_PCM_ALAW.  Another format, a null pointer or n != 256 (expand) is NUTLS_ERR_ARG, and nothing is written. */
int nutls_pcm_g711_expand(int sample_format, short* table, int n);
int nutls_pcm_g711_compress(int sample_format, const short* in, unsigned char* out, size_t n);
/* "Upper band" above.  gain in 0 .. 1, 0 = off (the default); NaN, a gain outside 0 .. 1, or a gain other than 0 at 8000 / 16000 Hz:
 * NUTLS_ERR_ARG, nothing changes.  Synchronises and zeroes every stream's resampler histories and upper-band state, unless the gain is the
 * one the handle already has.  nutls_set_pcm_format resets it to 0: call this after it. */
int nutls_set_pcm_upper_band(nutls_handle* h, float gain);
int nutls_pcm_upper_band(nutls_handle* h, float* gain);      /* the gain in force */
#define NUTLS_PCM_FOLLOW_HOPS 4   /* hops of the two energy windows of follow ("Upper band" above) */
int nutls_set_pcm_upper_follow(nutls_handle* h, int enable);   /* gain of nutls_set_pcm_upper_band becomes the CEILING of a gain that follows the model */
int nutls_pcm_upper_follow(nutls_handle* h, int* enable);
int nutls_pcm_follow_gain(nutls_handle* h, float* gains, int n);  /* HOST [rows]: g of each row's last real encoded hop; synchronous; 0 after reset */
int nutls_pcm_hop_samples(nutls_handle* h);     /* S = 256 * rate / 16000: 128, 256, 512, 768 */
int nutls_pcm_delay_samples(nutls_handle* h);   /* delay of the two rate conversions together, in samples at the caller's rate */
int nutls_pcm_filter_taps(int rate_hz);         /* host only, no handle: 2 K q + 1; 1 for 16000; -1 for an unsupported rate */
int nutls_pcm_filter(int rate_hz, float* taps, int n);   /* host only: the fp32 prototype filter the kernels use; n = nutls_pcm_filter_taps */
/* Streaming handles.  pcm_in / pcm_out: DEVICE [B, S] of the handle's sample type (HOST in the _host entries); `active` as in
 * nutls_enhance_hop_active (DEVICE [B] bytes, HOST in the _host entry; NULL = the entry without the mask); asynchronous on `stream`. */
int nutls_enhance_hop_pcm(nutls_handle* h, const void* pcm_in, void* pcm_out, int dc_mode, void* stream);
int nutls_enhance_hop_pcm_active(nutls_handle* h, const void* pcm_in, void* pcm_out, const unsigned char* active, int dc_mode, void* stream);
int nutls_enhance_hop_pcm_host(nutls_handle* h, const void* pcm_in, void* pcm_out, int dc_mode);
int nutls_enhance_hop_pcm_host_active(nutls_handle* h, const void* pcm_in, void* pcm_out, const unsigned char* active, int dc_mode);
/* The two halves on their own (testing, custom models), as nutls_stft_hop / nutls_istft_hop are: the callers' format <-> DEVICE [B, 256]
 * float32 at 16 kHz.  `active`: DEVICE mask or NULL; a held row of the output is zeros (of nutls_pcm_encode_hop in a G.711 format: the
 * silence code, 0xFF / 0xD5).  Any streaming handle. */
int nutls_pcm_decode_hop(nutls_handle* h, const void* pcm_in, float* hop_out, const unsigned char* active, void* stream);
int nutls_pcm_encode_hop(nutls_handle* h, const float* hop_in, void* pcm_out, const unsigned char* active, void* stream);
/* Offline handles (nutls_create_offline, nutls_create_offline_batch): DEVICE [utterances, n_hops * S] (HOST in the _host entry),
 * 1 <= n_hops <= max_frames; the 16 kHz side of the halves is [utterances, n_hops * 256] float32. */
int nutls_enhance_block_pcm(nutls_handle* h, const void* pcm_in, void* pcm_out, int n_hops, int dc_mode, void* stream);
int nutls_enhance_block_pcm_host(nutls_handle* h, const void* pcm_in, void* pcm_out, int n_hops, int dc_mode);
int nutls_pcm_decode_block(nutls_handle* h, const void* pcm_in, float* wave_out, int n_hops, void* stream);
int nutls_pcm_encode_block(nutls_handle* h, const float* wave_in, void* pcm_out, int n_hops, void* stream);
/* Ragged blocks in the callers' format: "Ragged blocks" above, with hops of S samples of the handle's sample type.  pcm_in / pcm_out:
 * [utterances, n_hops * S], base pointer 16-byte aligned; hops: [utterances] int, hops[u] = k in 0 .. n_hops LEADING real hops of utterance u.
 * nutls_enhance_block_pcm_ragged decodes with the counts, calls nutls_enhance_block_ragged on the library's float buffers and encodes with
 * the counts.  For utterance u, one call
 *   - writes hops 0 .. k-1 of pcm_out with exactly the bits nutls_enhance_block_pcm of the same width writes there;
 *   - writes hops k .. n_hops-1 of pcm_out with ZEROS (a G.711 format: with the silence code, 0xFF / 0xD5, not zero bytes); the matching hops
 *     of pcm_in are not read and may hold anything (NaN, any int16, any byte).  The caller's input buffer is never written;
 *   - carries the resampler history of both directions from hop k-1, and what nutls_enhance_block_ragged carries from frame k;
 *   - k = 0 HOLDS the utterance completely: both resampler histories, the previous hop, the overlap tail and the model state stay as they were.
 * Any cut of a recording into ragged calls gives the same concatenated samples, bit for bit.  hops == NULL: the call IS the entry without
 * counts (same code path, same bits).  At 16000 / NUTLS_PCM_F32 the two enhance entries ARE nutls_enhance_block_ragged / _ragged_host.
 * Device entries: hops is a DEVICE pointer that the kernels read and clamp to 0 .. n_hops (the host does not synchronise to look); it stays
 * valid and unmodified until the work queued on `stream` has run.  The _host entry takes pcm_in, pcm_out and hops in HOST memory; a count
 * outside 0 .. n_hops, a bad dc_mode or n_hops, a null pointer or a streaming handle is NUTLS_ERR_ARG (nutls_last_error says which), checked
 * before anything is converted: a refused call leaves every history where it was.  The two halves: nutls_pcm_decode_block /
 * nutls_pcm_encode_block with counts; the 16 kHz side is [utterances, n_hops * 256] float32, its hops behind a count are zeros (the callers'
 * side of the encode half in a G.711 format: the silence code).
 * Cost: the uniform entry's (the kernels return early behind a count; the model computes and discards, see "Ragged blocks"). */
int nutls_enhance_block_pcm_ragged(nutls_handle* h, const void* pcm_in, void* pcm_out, int n_hops, const int* hops, int dc_mode, void* stream);
int nutls_enhance_block_pcm_ragged_host(nutls_handle* h, const void* pcm_in, void* pcm_out, int n_hops, const int* hops, int dc_mode);
int nutls_pcm_decode_block_ragged(nutls_handle* h, const void* pcm_in, float* wave_out, int n_hops, const int* hops, void* stream);
int nutls_pcm_encode_block_ragged(nutls_handle* h, const float* wave_in, void* pcm_out, int n_hops, const int* hops, void* stream);
/* Packet mode (streaming handles): the callers' PACKETS in and out, re-framed into hops on the device.  The library's unit of time is the hop,
 * 16 ms; nothing on the wire arrives in hops -- RTP PCMU / PCMA packets are 20 ms (160 bytes), sometimes 10 or 30, WebRTC's audio processing
 * runs on 10 ms frames (480 samples at 48 kHz), Opus on 20 ms.  A handle is told ONCE how many samples its callers' packets have
 * (nutls_set_pcm_packet); nutls_enhance_packet_pcm then takes one packet per stream and returns one packet per stream, and everything between
 * them -- the per-stream FIFOs in front of the model and behind it, which streams have a whole hop at this tick, the masks that follow, the
 * second hop of a tick in which a stream has two ready -- happens on the device, with no synchronisation in the device entry.
 *   Arithmetic (the contract).  S = nutls_pcm_hop_samples, P = the packet's samples at the callers' rate, g = gcd(P, S).  Every stream has an
 *   input FIFO, which starts empty, and an output FIFO, which starts with D = S - g samples of silence (zeros; in a G.711 format the law's
 *   silence code, 0xFF / 0xD5).  One call is a TICK.  For every stream whose `active` byte is non-zero it
 *     1. pushes the stream's P samples onto its input FIFO;
 *     2. while the input FIFO holds at least S samples: takes the oldest S, runs one hop of the existing pipeline on them -- exactly
 *        nutls_enhance_hop_pcm_active with a mask of the streams that are ready in this ROUND -- and appends the S results to the output FIFO;
 *     3. pops P samples from the output FIFO into the stream's row of pcm_out.
 *   For a stream that is HELD at the tick nothing of it changes -- FIFOs, resampler history, previous hop, overlap tail, model state --, its
 *   row of pcm_in is not read and its row of pcm_out is silence.
 *   D is the smallest priming with which step 3 never underruns; after every tick fill_in + fill_out = D, so one counter per stream describes
 *   both FIFOs; neither ever holds more than S - g + P samples; a tick runs at most R = floor((S - g + P) / S) rounds.
 *   So the concatenation of a stream's returned packets is D samples of silence followed by the concatenation of what nutls_enhance_hop_pcm
 *   returns for the stream's concatenated input cut into hops -- bit for bit, whatever the packet length, whichever ticks the stream was
 *   held at, whenever it joined and whoever shares the handle.  The total delay is D plus the one hop of nutls_enhance_hop plus
 *   nutls_pcm_delay_samples.
 *   Buffers: pcm_in / pcm_out are [B, P] of the handle's sample type, rows contiguous, base pointer 16-byte aligned.  `active` as in
 *   nutls_enhance_hop_pcm_active: DEVICE [B] bytes in nutls_enhance_packet_pcm, HOST memory in the _host entry, NULL = all streams.  The device
 *   entry is asynchronous on `stream`; the _host entry copies the packets through library buffers and synchronises, like the other _host
 *   entries of this section.
 *   Accepted packet lengths: P * bytes per sample is a multiple of 16 (rows stay 16-byte aligned, and every FIFO position is), and
 *   1 <= P <= 4 S, so R <= 4.  Everything else is NUTLS_ERR_ARG and changes nothing.  nutls_pcm_packet_plan states the rule on the host, with
 *   no handle and no GPU, as nutls_pcm_filter_taps does: delay = D, rounds = R, fifo = S - g + P (each pointer may be NULL); it knows the
 *   formats' rules (G.711 at 8000 only; an unknown rate or format is NUTLS_ERR_ARG).
 *   nutls_set_pcm_packet(h, P), 0 = off (the default), may be called between any two ticks.  Like the other switches of this section it
 *   synchronises the device; then it re-primes every stream's FIFOs -- input empty, output D samples of silence.  It does not touch the
 *   resampler histories, the model state or the upper band.  Setting the value in force is a no-op that touches nothing.
 *   nutls_set_pcm_format turns packet mode OFF, because a new format starts anew and S changes: set the packet length after the format.
 *   nutls_reset(h, b) re-primes stream b's FIFOs with everything else of the stream, -1 everybody's.  Packet mode changes nothing about the hop
 *   entries: they neither read nor write the FIFOs.  A packet call while the mode is off is NUTLS_ERR_ARG.
 *   nutls_pcm_packet_samples = P (0 when off), nutls_pcm_packet_delay_samples = D, nutls_pcm_packet_fill(h, fill, B) = HOST fill[B], the
 *   samples waiting in each stream's input FIFO, read from the device (synchronises; NUTLS_ERR_ARG while the mode is off or with n other than
 *   B), nutls_pcm_packet_last_rounds = the hop rounds the last packet call issued.
 *   Where: streaming handles; an offline handle is refused (its block entries take any number of hops).  When P is not a multiple of S, or when a
 *   mask is passed, the rounds are masked hops: packet mode is then refused exactly where nutls_step_active refuses a mask, with its reason
 *   (the baseline variant, NUTLS_CTFA_CAUSAL32, modes 0 / 1) -- checked before anything is pushed, at nutls_set_pcm_packet and again at every
 *   call, because the mode can change in between: a refused call changes nothing.  With P a multiple of S and no mask it works wherever
 *   nutls_enhance_hop_pcm does.  Hop fusion, the attenuation limit, the upper band and follow come with the hop entry.
 *   How many rounds a tick issues: a round nobody is ready for is not free (every held stream costs the state copy of nutls_step_active), so
 *   the library does not issue one where it can know.  The device keeps the per-stream counters and forms each round's ready mask itself; the
 *   host keeps a mirror of the same integers for as long as it sees the masks -- active == NULL, or the _host entry -- and issues exactly the
 *   rounds in which some stream is ready, possibly none; those rounds' masks also feed the bookkeeping behind nutls_state_set that the float
 *   _host entries do.  With a DEVICE mask the library cannot follow, and from then on every tick issues R rounds (the more expensive
 *   launches) until nutls_reset(h, -1) or nutls_set_pcm_packet -- the rule of nutls_step_active for masks the host has not seen.
 *   Cost: a tick of r rounds is r hops of nutls_enhance_hop_pcm_active and r + 1 small launches that move the packets; measured: README, "Packet mode". */
int nutls_pcm_packet_plan(int rate_hz, int sample_format, int samples, int* delay, int* rounds, int* fifo);  /* host only, no handle */
int nutls_set_pcm_packet(nutls_handle* h, int samples);      /* 0 = off (the default) */
int nutls_pcm_packet_samples(nutls_handle* h);               /* P, 0 when off */
int nutls_pcm_packet_delay_samples(nutls_handle* h);         /* D */
int nutls_pcm_packet_fill(nutls_handle* h, int* fill, int n);/* HOST [B]: samples waiting in each input FIFO, read from the device; synchronises */
int nutls_pcm_packet_last_rounds(nutls_handle* h);           /* hop rounds the last packet call issued */
int nutls_enhance_packet_pcm(nutls_handle* h, const void* pcm_in, void* pcm_out, const unsigned char* active, int dc_mode, void* stream);
int nutls_enhance_packet_pcm_host(nutls_handle* h, const void* pcm_in, void* pcm_out, const unsigned char* active, int dc_mode);

/* ---- Channels: interleaved 2- and 4-channel audio, one stream per channel ----------------------------------------------------------
 * The audio the formats above were built for rarely arrives one row per talker: a call-centre archive is a stereo file with the agent on the
 * left and the customer on the right, a WebRTC or Opus decoder hands over interleaved stereo, a wave-file reader returns [N, C].  The channels
 * of such a frame are what a handle's streams are -- independent talkers with their own model state --, so a handle can be told that its
 * callers' buffers hold C channels per frame, and the split and the join happen on the device, beside the conversions.
 *   The layout (the contract).  B is the handle's rows: the streams of a streaming handle, the utterances of an offline one.  While C > 1
 *   the callers' side of EVERY _pcm entry is [B / C, n * C] of the handle's sample type, and sample i of stream r * C + c is at column
 *   i * C + c of row r: channel c of frame row r is stream r * C + c.  This covers the four hop entries, nutls_pcm_decode_hop /
 *   nutls_pcm_encode_hop, the block entries and their halves, the _ragged forms, nutls_enhance_packet_pcm and its _host form; n is S
 *   (nutls_pcm_hop_samples), n_hops * S or P.  The base pointer is 16-byte aligned as before; rows stay multiples of 16 bytes because
 *   S * bytes and P * bytes already are.  The 16 kHz float side of the halves stays [B, 256] and [utterances, n_hops * 256], one row per stream.
 *   Everything else is per stream, as it was: `active` is [B] bytes, `hops` is [B] counts -- the channels of one frame row may have different
 *   counts, 0 included --, and the attenuation limit, nutls_pcm_follow_gain, nutls_pcm_packet_fill and nutls_reset(h, b) work per stream.
 *   A held stream's samples, and the hops behind a count, now sit in the same 16-byte words as their partner's: they are read as bytes,
 *   HAVE NO EFFECT and may hold anything, NaN included (where this header says "is not read" of such samples, read "has no effect" while
 *   C > 1).  On the way out they carry what the 1-channel entry writes there: zeros, or the law's silence code 0xFF / 0xD5.
 *   THE RULE: for every entry E, E_C(x) == interleave(E_1(deinterleave(x))) in every bit -- outputs and all carried state.
 *   nutls_set_pcm_channels(h, C): 1 = off (the default), 2 or 4, which need B % C == 0.  Any other value, a B that C does not divide or a
 *   null handle is NUTLS_ERR_ARG; nutls_last_error names the entry and nothing changes.  It is a setting, not stream state, like the
 *   attenuation limit: it may be called between any two calls, synchronises the device, touches no history, FIFO, model state, upper-band
 *   or follow state, and survives nutls_reset and nutls_set_pcm_format.  So a stream's concatenated output does not depend on the layout its
 *   hops arrived in, and the layout may change in mid-stream.  Setting the value in force is a no-op.  nutls_pcm_channels = C.
 *   pcm_in == pcm_out (the same base pointer) stays allowed: the input is split into a library buffer before anything writes the output.
 *   With C == 1 every entry launches exactly the kernels it launched before this section existed, same bits.  With C > 1 an entry is a
 *   split launch, the 1-channel entry on library buffers, a join launch -- at 16000 / NUTLS_PCM_F32 too, where the 1-channel entry is the
 *   plain float one.  Refusals are checked before anything is split: a refused call changes nothing.  The _host entries copy the interleaved
 *   bytes through their staging (the byte count is the same) and take the device path.  The plain float entries (nutls_enhance_hop,
 *   nutls_enhance_block, the nutls_stft_ and nutls_step families) ignore the setting, as they ignore the format.
 *   nutls_pcm_deinterleave / nutls_pcm_interleave are the library's statement of the rule, host only, with no handle and no GPU, as
 *   nutls_pcm_g711_expand is: frames [n, C] -> rows [C, n] and back, samples of 4, 2, 1, 1 bytes for NUTLS_PCM_F32, _S16, _ULAW, _ALAW, moved as
 *   bytes.  Any n >= 0 is accepted; the two buffers must not overlap.  Channels other than 2 or 4, an unknown format or a null pointer is
 *   NUTLS_ERR_ARG and nothing is written.  The kernels agree with them bit for bit.
 *   Cost: two small launches per call, which move every byte once each way; measured: README, "Channels". */
int nutls_set_pcm_channels(nutls_handle* h, int channels);   /* 1 = off (the default), 2 or 4 */
int nutls_pcm_channels(nutls_handle* h);
int nutls_pcm_deinterleave(int sample_format, int channels, const void* frames, void* rows, size_t n);  /* host only, no handle: [n, C] -> [C, n] */
int nutls_pcm_interleave(int sample_format, int channels, const void* rows, void* frames, size_t n);    /* host only, no handle: [C, n] -> [n, C] */

/* ---- Attenuation limit: a per-row cap on how much noise is removed ------------------------------------------------------
 * Every waveform entry returns the model's full suppression by default.  With a limit l in 0 .. 1 on a row (a stream of a streaming handle,
 * an utterance of an offline one) the synthesis mixes, per bin 1..256 of every frame, the noisy magnitude x of that frame (as the analysis
 * wrote it) with the model's magnitude e of the same frame, on the frame's own phase:
 *     m' = fma(l, x, c * e),   c = (float)(1.0 - (double)l) formed once on the host,
 * the product c * e and the fma rounded separately.  Both magnitudes share the phasors and the synthesis is linear, so the samples are
 * (1 - l) * enhanced + l * noisy, aligned, with no delay line and no extra launch; since e >= 0 no bin is attenuated below l * x, i.e. by more
 * than -20 log10(l) dB.  The DC rule (dc_mode) applies to m' as it applied to e.
 *   - Exact ends: l = 0 (the default) gives m' = e bit for bit, l = 1 gives m' = x bit for bit (the input through analysis and synthesis).
 *   - A setting, not stream state: it survives nutls_reset, nutls_set_pcm_format and mode switches.  The kernels read it from a per-row
 *     device array, so a change holds from the next call.  A row held by an `active` mask or behind a ragged count behaves as before: a zero
 *     hop, its overlap tail kept, no input row read.
 *   - Kernels: while EVERY row of a handle is 0 every entry launches exactly the kernels it launches without this section -- same bits.  As
 *     soon as one row is not 0 the synthesis of every launch is its mix twin, and the rows at 0 go through it with (l, c) = (0, 1).
 *   - Who honours it: nutls_istft_hop (noisy rows = the library's mag_in buffer as the last nutls_stft_hop left it) and with it every
 *     nutls_enhance_hop* entry -- device, _host, _active, _pcm*; nutls_enhance_block, _ragged, their _host forms and the _pcm* block entries
 *     (noisy rows = the library's mag_in buffer); nutls_istft_block_mix.  Who does not: nutls_istft_block[_ragged], which have no noisy rows
 *     (nutls_stft_block wrote them to the caller's buffer) and stay exactly as they are, and the magnitude entries nutls_step* and
 *     nutls_process_block* -- a caller who holds both rows mixes them itself.
 *   - Hop fusion: the one-launch hop builds have no mix.  nutls_set_atten_limit with a value other than 0 on a handle in hop fusion, and
 *     nutls_set_hop_fusion(h, nonzero) while a row's limit is not 0, are NUTLS_ERR_ARG and change nothing; an all-zero set is accepted.
 *   - PCM gateway: decode and encode sit around the plain hop or block and get the limit through it.  The upper band's follow mode
 *     (nutls_set_pcm_upper_follow) then follows the LIMITED suppression: its B_t is the energy of what the encode half is handed.
 * nutls_set_atten_limit(h, limit, n): limit is a HOST array of n = the handle's rows (streams / utterances) floats; NULL sets every row to 0.
 * A value outside 0 .. 1, a NaN or a wrong n is NUTLS_ERR_ARG (nutls_last_error names the entry) and changes nothing.  A CONTROL-PLANE call,
 * like nutls_offline_set_ctfa_mode: it synchronises the device, then writes the per-row (l, c) array -- not for the audio path's inner loop.
 * nutls_atten_limit(h, limit, n): HOST limit[rows] = the l in force. */
int nutls_set_atten_limit(nutls_handle* h, const float* limit, int n);
int nutls_atten_limit(nutls_handle* h, float* limit, int n);
/* The synthesis half of the waveform block mode with the noisy rows in the caller's hands: est, noisy DEVICE [utterances, n_hops, 256] (noisy
 * as nutls_stft_block[_ragged] wrote it), hops DEVICE [utterances] counts as in nutls_istft_block_ragged or NULL for the uniform block.
 * Otherwise nutls_istft_block[_ragged]; with every limit 0 it launches their kernels and never reads noisy. */
int nutls_istft_block_mix(nutls_handle* h, const float* est, const float* noisy, float* pcm_out, int n_hops, const int* hops, int dc_mode, void* stream);

/* ---- Non-finite input: what a live row that goes bad may do to the others, and how it heals ---------------------------------------
 * One handle serves many callers.  A workgroup steps two or four streams side by side, a per-layer tile of 128 positions spans several
 * streams, in block mode a tile spans several frames and utterances, one stereo frame row carries two talkers, the corpus scheduler hands a
 * slot to the next recording.  A row is a stream of a streaming handle or an utterance of an offline one.  "Poison" is anything a LIVE
 * row is fed that is not a finite number that stays finite: NaN, +-Inf, or finite values that overflow inside (a magnitude row of 3e38).
 * (A HELD row and the rows behind a ragged count may hold anything because they have no effect; that is said where those are defined.)
 *   1. Containment across rows.  Whatever one row is fed, EVERY OTHER ROW of the handle is bit-identical to the run in which that row was
 *      fed zeros instead: outputs, all state tensors of nutls_state_get, and every per-row library state (previous hop, overlap tail,
 *      resampler histories, upper band, nutls_pcm_follow_gain, nutls_pcm_packet_fill, the causal32 attention history).  On every entry,
 *      plan (1, 2, 4 streams per workgroup), mode (0, 1, 3), variant, CTFA mode, with nutls_debug_trace on or off, hop fusion on or off, in
 *      the callers' formats, with channels and packets.  No row is ever combined with another under a weight or a mask of zero: 0 x NaN
 *      is NaN, so "excluded" means not read, or selected away, never multiplied away.
 *   2. Containment in time (block entries).  Every layer is causal in time: poison in frame t of an utterance leaves that utterance's
 *      output rows 0 .. t-1 of the call (and everything earlier calls returned) bit-identical to the clean run.  Waveform entries: input
 *      hop t makes frames t and t + 1, and output hop t is the first half of synthesis block t plus the second half of block t - 1; so
 *      poison in input hop t leaves output hops 0 .. t-1 -- samples 0 .. 256 t - 1 of the utterance -- bit-identical, and output hop t, which
 *      carries the signal of input hop t - 1 (the one-hop lag), is the first that may differ.  In the callers' format the same holds with
 *      the decode half's window below in front: caller's sample n reaches 16 kHz sample ceil(n / q) at the earliest.
 *   3. Finite support of the stateless halves.  The transforms, the resamplers, the upper band and follow have no recurrence: through
 *      nutls_stft_hop / nutls_istft_hop, nutls_stft_block / nutls_istft_block, nutls_pcm_decode_* / nutls_pcm_encode_* ALONE one poisoned
 *      input sample may change only the outputs inside the windows below; every output outside is bit-identical to the clean run, and the
 *      row is finite again behind the window.  T = nutls_pcm_filter_taps(rate), L = T - 1, q = max(rate, 16000) / min(rate, 16000),
 *      S = nutls_pcm_hop_samples, W = NUTLS_PCM_FOLLOW_HOPS; L = nutls_pcm_delay_samples above 16 kHz and twice that at 8 kHz; all windows
 *      closed, samples counted along the row's concatenated hops since its last reset:
 *        rate reduction by q (decode above 16 kHz, encode at 8 kHz)   sample n -> samples ceil(n / q) .. floor((n + L) / q)
 *        rate increase by q (decode at 8 kHz, encode above 16 kHz)    sample m -> samples q m .. q m + L
 *        decode then encode (the model the identity, no lag)          sample n -> samples n' .. n'' + 2 nutls_pcm_delay_samples, with n', n''
 *                                                                     = n rounded up, down to a multiple of q above 16 kHz, = n at 8 kHz
 *        analysis (nutls_stft_hop, nutls_stft_block)                  sample n -> magnitude and phasor frames floor(n / 256) and the next
 *        synthesis (nutls_istft_hop, nutls_istft_block)               frame f, a magnitude or a phasor -> samples 256 f .. 256 (f + 2) - 1
 *        analysis then synthesis (frame 512, hop 256)                 sample n -> the three output hops floor(n / 256) .. floor(n / 256) + 2
 *        upper band, u recorded by the decode half                    sample n -> u[n' .. n'' + 2 L], added by the encode half S samples
 *                                                                     later: output samples n' + S .. n'' + 2 L + S
 *        follow, energy a_s of decoded hop s not finite                -> the whole output hops s + 1 .. s + W + 1 (A_t sums a_(t-1) .. a_(t-W),
 *                                                                     and gamma_t ramps from g_(t-1) to g_t)
 *        follow, energy b_s of an encoded hop s not finite             -> the whole output hops s .. s + W
 *      (fminf / fmaxf return their finite argument, so a NaN energy may give a finite gain: still inside the window.)
 *   4. Healing.  After nutls_reset(h, b) row b is bit-identical to the same row of a FRESH handle of the same configuration fed the same
 *      continuation, whatever the row held -- NaN and Inf included: everything a reset restarts is rewritten (memset: zeros, or the silence
 *      that primes a packet FIFO), never scaled by zero.  The same holds for the histories that nutls_set_pcm_format, nutls_set_pcm_upper_band, nutls_set_pcm_upper_follow,
 *      nutls_set_pcm_packet and a CTFA mode switch restart.  Rows that are not reset are untouched.  Without a reset a poisoned row stays
 *      poisoned for as long as its recurrent state is (NaN in an LSTM cell never decays).
 *   5. Not specified: what the poisoned row itself returns, beyond the rules above and those that already exist (NaN -> 0 -> the silence
 *      code on the int16 / G.711 encode).
 * tests/poison_reference.py states the windows, tests/test_poison_reference.py holds them against float64, tests/test_gpu_poison.py holds
 * the kernels to 1 - 4, bit for bit. */

/* Library-owned device staging buffers [B,256]; stepping on them avoids the D2D copies and lets
 * the captured hipGraph run with no per-call parameter update. */
int nutls_io_buffers(nutls_handle* h, float** mag_in, float** mag_out);

/* Execution mode of nutls_step:
 *   3            fused kernel: ONE launch per frame, one 512-thread workgroup per stream (per two / four streams where the library's
 *                cost model finds a packed plan faster -- more streams than CUs: nutls_streams_per_workgroup); every op of the step
 *                is its own specialised instruction stream (static schedule, no plan decoding).  Both variants
 *                have one; it keeps the conv kernels int8 on the device, so it exists for handles made from a
 *                container with int8 conv kernels (what the reference's .tflite stores) and is their default;
 *   1            one kernel per layer, the ~160 launches captured in a hipGraph (one per state parity);
 *   0            one kernel per layer, plain launches (handles made from containers without int8 conv kernels start in mode 1).
 * (2 was the plan-interpreter kernel of rounds 1-3; retired, nutls_set_mode(2) is an error.)  All of them compute the same function (tests/test_gpu_parity.py::test_execution_modes_agree). */
int nutls_set_mode(nutls_handle* h, int mode);
/* enable != 0: mode 1 (capture + replay); enable == 0: mode 0. */
int nutls_use_graph(nutls_handle* h, int enable);

/* State access by the reference's signature names.  `name` is any of the 130 state inputs
 * ("msfe6_ee_prev1" ... "msfe6_de_c", converter_proposed.py:27-186); the matching output spelling
 * ("..._cur1") is accepted as an alias.  Host buffer layout: [B, F, C] (conv states) or [B, 21],
 * float32, `n_floats` must equal B * per-stream size.  Synchronous.
 * (The fused kernel does not write the 40 conv-input states it never reads itself -- the echoes of the strided convs' inputs,
 * converter_proposed.py:226-231 -- on every frame: their rows exist a second time as skip-connection slices of other states, and the
 * library rebuilds them from there before any of the accessors below, a step of another mode or nutls_reset looks at the states.
 * What a caller sees is what the reference's runner returns, frame by frame; NUTLS_EAGER_STATES=1 makes every launch write everything.)
 * nutls_state_set and the causal32 CTFA of a streaming handle: the 31-frame time-attention history (nutls_set_ctfa_mode) is library state
 * outside the signature's tensors and nutls_state_set does not touch it -- the buffers are [B, ...], so "get, change stream b's row, set"
 * leaves the other B - 1 live streams exactly as they were.  To start a NEW utterance in stream b from loaded states, call
 * nutls_reset(h, b) first (zeroes b's states and its history), then set. */
int nutls_state_get(nutls_handle* h, const char* name, float* host_buf, size_t n_floats);
int nutls_state_set(nutls_handle* h, const char* name, const float* host_buf, size_t n_floats);

/* Every state tensor of ONE stream, concatenated in nutls_state_info order (n_floats = sum of the per-stream sizes):
 * what the signature runner hands back per frame, with a single device-to-host copy. */
int nutls_state_get_all(nutls_handle* h, int stream_idx, float* host_buf, size_t n_floats);

/* Enumerate the state tensors: count, then name + per-stream dims (F, C) or (21, 1). */
int nutls_state_count(nutls_handle* h);
int nutls_state_info(nutls_handle* h, int index, const char** name, int* dim0, int* dim1);

/* Zero the state of one stream (stream_idx >= 0) or of all streams (stream_idx < 0): the
 * all-zero seed of interpreter_proposed.py:36-198. */
int nutls_reset(nutls_handle* h, int stream_idx);

/* Copy the last step's value of an internal activation to the host (testing / debugging):
 * "<stage>.y" (CTFA output [B,F0,64]), "<stage>.up" (decoder up-sampled input [B,F0,128]),
 * "input_layer" ([B,256,64]).  Per-layer modes (0 / 1): the last stage's tensors ("msfe6_de.y", "msfe6_de.up": the layers share one scratch
 * tensor per kind) and "input_layer".  Fused mode: these tensors never leave LDS; with nutls_debug_trace(h, 1) every step of a one-stream
 * fused handle (<= 64 streams) runs on the library's profiling build of the step kernel, which copies them out -- "<stage>.y" of all 12
 * stages, "<stage>.up" of the 6 decoder stages, "input_layer" of the LAST step -- for layer-by-layer comparison with a reference trace
 * (tests/test_gpu_trace.py).  Testing / debugging only: the profiling build is a few percent slower.
 * Offline handles, waveform block mode: "phasor_block" = the unit phasors of the last analysed block, [utterances, its n_hops, 257, 2]. */
int nutls_debug_trace(nutls_handle* h, int enable);
/* Developer knobs of a handle (timing experiments; no effect on results).  "skew": start skew of the fused kernel's workgroups -- workgroup w
 * sleeps (w mod 4) * value * 64 clocks before its first op (0 = off, the default; NUTLS_FUSED_SKEW sets it at creation).  Experiment builds
 * of the step kernel (tools/exp/build_plan_lib.sh ... -DFZ_STOPAT=1) read the same field as "stop after this many ops", which is how
 * tools/exp/prod_timeline.py times variants of the UN-instrumented kernel op by op (the library's own kernel: nutls_profile_production).
 * Unknown names: NUTLS_ERR_ARG. */
int nutls_debug_knob(nutls_handle* h, const char* name, int value);
int nutls_debug_get(nutls_handle* h, const char* name, float* host_buf, size_t n_floats);

int nutls_batch(nutls_handle* h);
/* Streams one workgroup of the fused kernel steps (mode 3): 1, or -- LSTM variant, more streams than CUs -- 2 or 4: a packed plan
 * (csrc/fused_step_g2.hip / _g4.hip: the layers whose LDS images fit that often run the streams side by side on one position axis, sharing
 * the weight fetch and conversion; chosen by nutls_create so that rounds of workgroups x step time of the plan is smallest -- with 256 CUs:
 * 256 streams 1, 300 .. 512 2, 768 1, 1024, 1536 and 2048 2; the four-stream plan on request).  A stream's results do not depend on its slot or partners.
 * NUTLS_FUSED_STREAMS=1 at creation keeps the one-stream plan; nutls_create_plan chooses explicitly.  No reference counterpart (the reference steps one stream: interpreter_proposed.py:215). */
int nutls_streams_per_workgroup(nutls_handle* h);
int nutls_launches_per_step(nutls_handle* h);

/* Introspection of the per-frame launch plan (nutls_launches_per_step entries, in issue order):
 * layer name (reference Keras layer, e.g. "msfe6_en_spconv6"), kernel family (one family = one
 * kernel symbol), and the ALGORITHMIC work of that launch for the handle's batch:
 * flops = 2 * MACs, bytes = 4 * (input elements read incl. the previous-frame tap + output
 * elements written)  -- the "layer-fused" traffic model of SURVEY.md section 8(d). */
int nutls_launch_info(nutls_handle* h, int index, const char** layer, const char** family,
                      double* flops, double* bytes);
/* The conv launches of that plan: kind (0 .. 9: el_c32, el_c64, el_c128, dl_n64, dl_n128, in_c64, in_c128, down, up_even, up_odd) and output
 * positions per stream; kind = -1, f_out = 0 for a launch that is no conv.  The block plan of an offline handle has the same entries. */
int nutls_launch_conv_shape(nutls_handle* h, int index, int* kind, int* f_out);
/* Which instantiation of the per-layer conv kernels a launch of `batch` streams (block mode: utterances x frames of the launch) x `f_out`
 * positions of that kind runs -- the library's one rule, the function its launches dispatch on.  Host only: no handle, no device.
 * bf16 != 0: conv_bf16x3_kernel (block mode on an int8 container), else conv_mfma_kernel.  ksplit / tile_min: the developer knobs
 * NUTLS_OFFLINE_KSPLIT (default 1) and NUTLS_CONV_TILE_MIN (positions per launch from which the 128-position tiles run; < 0: the
 * defaults, 32768 bf16 / 65536 fp32), which a handle reads from the environment when it is created.
 * Out (each may be null): template arguments NW and ALL ((4, 1) = the K split; fp32: all = 0), positions per workgroup (32 / 128),
 * workgroups (the last one partly filled where batch * f_out is no multiple of the tile), bytes of dynamic LDS. */
int nutls_conv_dispatch(int kind, int batch, int f_out, int bf16, int ksplit, long long tile_min, int* nw, int* all, int* tile,
                        long long* grid, long long* lds_bytes);

/* Run ONE step with plain launches on the library's own stream, bracketing every launch with
 * HIP events recorded on that stream; writes the milliseconds of each launch to ms[0..n).
 * Advances the state like nutls_step (input = the library's mag_in buffer).  Synchronous. */
int nutls_profile_step(nutls_handle* h, float* ms, int n);

/* Fused-mode twin: op count / names / algorithmic flops per stream of a variant's static schedule, and one profiled
 * step (workgroup 0 stamps every op boundary); microseconds per op to us[0..nutls_fused_num_ops(variant of h)). */
int nutls_fused_num_ops(int variant);
int nutls_fused_op_info(int variant, int index, const char** name, double* flops);
int nutls_profile_fused(nutls_handle* h, double* us, int n);
/* The same timeline from the UN-instrumented instruction stream (one-stream plan of the LSTM variant): the library's "stop twin" of the step
 * kernel -- the production code plus one scalar compare per op -- ends a launch in front of op N; cum_us[N], N = 0 .. nutls_fused_num_ops (= the
 * whole step), is the time per launch of `steps` back-to-back launches that end there (best of `reps` windows, HIP events), so
 * cum_us[N + 1] - cum_us[N] is what op N adds to the production kernel: no stamps on the critical wave, and every workgroup under the load of all the
 * others (the profiling build's workgroup 0 runs in their wake).  cum_us[0] is the launch floor.  n must be nutls_fused_num_ops + 1.  Timing
 * only: the truncated launches leave the streams between two frames, every stream is reset afterwards (input: the library's mag_in buffer). */
int nutls_profile_production(nutls_handle* h, double* cum_us, int n, int reps, int steps);
/* Host-only (works without a GPU): the fused kernel's weight blob for a container -- conv kernels int8 in MFMA fragment
 * order, everything else fp32, in the order of the variant's static schedule.  n_floats must equal
 * nutls_fused_blob_floats(variant). */
int nutls_fused_blob_floats(int variant);
int nutls_fused_pack_blob(const void* weights, size_t n_bytes, int variant, float* out, size_t n_floats);
/* The same for the plan with `streams` streams per workgroup (1: the two entries above; 2: the packed plan of the LSTM variant, whose
 * tilings -- hence fragment order -- differ); nutls_fused_plan_blob_floats is 0 where no such plan exists. */
int nutls_fused_plan_blob_floats(int variant, int streams);
/* Op instances of that plan (a packed plan has one instance of a layer per group of streams that runs it side by side: "name#s2" = the
 * instance that starts at stream slot 2) -- the count nutls_profile_fused expects for a handle on that plan. */
int nutls_fused_plan_num_ops(int variant, int streams);
int nutls_fused_plan_op_info(int variant, int streams, int index, const char** name, double* flops);
int nutls_fused_pack_blob_plan(const void* weights, size_t n_bytes, int variant, int streams, float* out, size_t n_floats);

const char* nutls_last_error(void);
const char* nutls_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NUTLS_H_ */
