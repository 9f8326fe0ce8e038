/*
 * gnsscorr.h — C-ABI of libgnsscorr.so, the MI355X (gfx950) replacement for the hot path of
 * gnsscusdr/CU-SDR-Collection (reference @ 2024_10_08, 100 % MATLAB).
 *
 * The reference has no FFI boundary of its own: the boundary is cut *inside*
 * two MATLAB functions and every entry point below names the reference lines it replaces
 * (paths relative to the reference root; "L1CA/" = GPS/GPS_L1CA/).
 *
 *   tracking.m:226-236   fread + int8->double + de-interleave      -> gc_load_if / gc_attach_if
 *   tracking.m:156-158   padded code table [c(L) c c(1)]           -> gc_set_channel / gc_set_code
 *   tracking.m:247-300   replica ramps, carrier, mix, six sums     -> gc_correlate (+ replay API)
 *   tracking.m:133-368   channel x epoch loops incl. loop closure  -> gc_track  (host C++ filters)
 *   acquisition.m:151-200  sigPower, coarse PCPS search, peak pick -> gc_acquire_coarse
 *   acquisition.m:206-254  fine-frequency search                   -> gc_acquire_fine
 *
 * Conventions: plain C types only; status-code returns (0 = OK, negative = error, text via
 * gc_last_error()); no exceptions cross the ABI; caller-owned host buffers are never retained
 * past the call that receives them; a context is used by one host thread at a time.
 * There is NO CPU fallback: every compute entry point runs HIP kernels on the context's
 * device and fails with GC_E_HIP if that is impossible.
 */
#ifndef GNSSCORR_H
#define GNSSCORR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GC_API_VERSION 4 /* 4: gc_acq_shift_pick.peak / second_peak are doubles (float64 guard); gc_device_count, gc_acq_guard_stats */

typedef struct gc_context gc_context;

enum gc_status {
  GC_OK = 0,
  GC_E_INVALID = -1,     /* bad argument */
  GC_E_RANGE = -2,       /* a block reaches past the loaded IF buffer (tracking.m:241-245) */
  GC_E_NOMEM = -3,
  GC_E_HIP = -4,         /* HIP runtime / device failure */
  GC_E_STATE = -5,       /* call sequence error (no IF loaded, channel not configured ...) */
  GC_E_UNSUPPORTED = -6
};

/* settings.dataType ('schar' | 'int16'), initSettings.m:60 */
enum gc_dtype { GC_I8 = 0, GC_I16 = 1 };
/* settings.fileType (1 = real, 2 = I/Q interleaved), initSettings.m:62-65; GC_QI is the
 * GLONASS sample order (GLO_GL1/include/tracking.m:227). */
enum gc_layout { GC_REAL = 0, GC_IQ = 1, GC_QI = 2 };

#define GC_MAX_ARMS 3
#define GC_TAPS 3  /* early, prompt, late */

/* ---- lifetime ---------------------------------------------------------------------- */
int gc_create(gc_context** ctx, int device_id);
int gc_destroy(gc_context* ctx);
const char* gc_last_error(void);
/* What this library was built as.  GC_BUILD_TUNING: libgnsscorr_tuning.so (-DGC_TUNING=1) - the kernels' A/B switches of
 * docs/KNOBS.md are live environment variables and the experimental kernels are linked in; the library that ships reads none. */
enum { GC_BUILD_TUNING = 1 };
int gc_build_flags(void);
int gc_api_version(void);
/* Device name / CU count of the context's device (for bench reporting). */
int gc_device_info(gc_context* ctx, char* name, int name_len, int* compute_units);
/* How many HIP devices this process sees (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES applied): the valid device_id of gc_create are
 * 0 .. *count - 1 (gc_create refuses an ordinal that is not gfx950).  0 without a driver or a device; needs no context.  The caller that shards channels over the GPUs of a node (tracking.m:133: channels are independent) makes
 * ONE context per device - gc_create(&ctx[i], i), i < *count - instead of SURVEY 8b's gc_create(ctx**, device_ids, ndev): a context
 * is bound to one device, one stream and one host thread ("deviations from SURVEY 8b"). */
int gc_device_count(int* count);
int gc_synchronize(gc_context* ctx);

/* ---- IF samples -> HBM (replaces fread + conversion, tracking.m:226-236) ------------ */
/* Copies `nsamples` samples (complex samples for IQ/QI, real samples for REAL) of raw
 * integers to the device.  The raw bytes stay as they are in HBM; conversion happens in
 * the kernels.  Replaces any previously loaded buffer. */
int gc_load_if(gc_context* ctx, const void* samples, uint64_t nsamples, int dtype, int layout);
/* 2-bit sign-magnitude packed complex records (two samples per byte; the reference converts them to schar files on
 * the CPU with GPS_L5C/include/unpack_cplx.m:32-49): upload the packed bytes and expand them on the GPU into the
 * int8 I/Q record (2 * nbytes samples).  SURVEY.md §8f item 2. */
int gc_load_if_packed2(gc_context* ctx, const void* packed, uint64_t nbytes);
/* As gc_load_if, reading from a file: `skip_bytes` as postProcessing.m:74
 * (fseek(fid, dataAdaptCoeff*skipNumberOfBytes)); nsamples = 0 reads to end of file. */
int gc_open_if_file(gc_context* ctx, const char* path, uint64_t skip_bytes, uint64_t nsamples,
                    int dtype, int layout);
/* Zero-copy: adopt a device pointer that already holds the raw samples (not owned). */
int gc_attach_if(gc_context* ctx, void* device_ptr, uint64_t nsamples, int dtype, int layout);
/* Device pointer and size of the current IF buffer (for tools that fill it in place). */
int gc_if_buffer(gc_context* ctx, void** device_ptr, uint64_t* nsamples);
/* sample type and order of the loaded record (GC_I8 / GC_I16, GC_IQ / GC_QI / GC_REAL) */
int gc_if_format(gc_context* ctx, int* dtype, int* layout);
/* Allocate an uninitialised device IF buffer owned by the context. */
int gc_alloc_if(gc_context* ctx, uint64_t nsamples, int dtype, int layout);
/* Read back raw samples [first, first+n) to the host (tests, CPU-baseline sampling). */
int gc_read_if(gc_context* ctx, uint64_t first, uint64_t n, void* dst);

/* ---- code replicas (replaces tracking.m:156-158) ------------------------------------ */
/* Declares a tracking channel: `arms` code arms (1 = data only; 2 = data+pilot,
 * GPS_L5C/include/tracking.m:151-160; 3 = B1C wide-band, BDS/B1C/include/WB_tracking.m:176-188)
 * whose index ramps are multiplied by `index_scale` R (1; 2 for BOC(1,1) / RZ tables,
 * GAL_E1C/include/tracking.m:236-262). */
int gc_set_channel(gc_context* ctx, int channel, int arms, double index_scale);
/* Padded table exactly as the reference builds it ([c(end) c c(1)], values in {-1,0,+1});
 * `arm_mult` is the extra factor applied to the ramp of this arm before ceil()
 * (6 for the BOC(6,1) arm, WB_tracking.m:293; otherwise 1). */
int gc_set_code(gc_context* ctx, int channel, int arm, const int8_t* table, int n_entries,
                double arm_mult);
/* Optional: stage only `window_entries` table entries (starting at the block's table_offset)
 * into LDS — needed for the 1 534 502-entry GPS L2C CL table, of which one block touches
 * 2*codeLength+2 entries (GPS_L2C/include/tracking.m:261).  0 = whole table (default). */
int gc_set_code_window(gc_context* ctx, int channel, int arm, int window_entries);

/* ---- correlator (replaces tracking.m:247-300) --------------------------------------- */
/* One integrate-and-dump block = the five scalars the reference records per epoch
 * (tracking.m:212-216,249,277,314,332) + block geometry.
 * The fields of a descriptor that are accepted (other values are GC_E_INVALID, samples beyond the IF buffer GC_E_RANGE; a channel
 * that is not configured, a missing table, record or sampling frequency are GC_E_STATE): blksize >= 1, first_sample >= 0,
 * code_phase_step > 0, el_spacing >= 0, rem_code_phase > -1, finite carr_freq and rem_carr_phase, and for every arm a
 * (R = index_scale, m_a = arm_mult, counted from the entry table_offset[a] names, where the staged table starts):
 *   el_spacing * R * max_a(m_a) < 1,
 *   (rem_code_phase - el_spacing) * R * m_a > -1        the early ramp's first index ceil(.) is >= 0: MATLAB index >= 1,
 *                                                       where tracking.m would stop with an index error on 0,
 *   ceil(((blksize - 1) * code_phase_step + rem_code_phase + el_spacing) * R * m_a) inside the table (or its window). */
typedef struct gc_block {
  int32_t channel;          /* index given to gc_set_channel */
  int32_t blksize;          /* N, tracking.m:222 */
  int64_t first_sample;     /* 0-based sample index of the block start in the IF buffer
                               (ftell/dataAdaptCoeff, tracking.m:212-216) */
  double rem_code_phase;    /* remCodePhase  (chips),   tracking.m:249 */
  double code_phase_step;   /* codeFreq/fs,             tracking.m:219 */
  double el_spacing;        /* earlyLateSpc (chips),    tracking.m:94  */
  double carr_freq;         /* carrFreq (Hz),           tracking.m:314 */
  double rem_carr_phase;    /* remCarrPhase (rad),      tracking.m:277 */
  int32_t table_offset[GC_MAX_ARMS]; /* per-arm index offset (GPS_L2C tracking.m:261) */
  int32_t reserved;
} gc_block;

/* Test hook: non-zero forces the generic correlator kernel (per-sample table lookup) even where the
 * fast single-transition kernel applies, so both can be checked against the oracle. */
int gc_force_generic_kernel(gc_context* ctx, int on);

/* Arithmetic of the correlations behind gc_correlate and every tracking entry point (gc_track, gc_track_resume,
 * gc_track_file, gc_track_device, gc_track_multi through each job's context).  GC_PREC_F32 (the default): the float32
 * kernels.  GC_PREC_F64: one float64 per-sample kernel (csrc/corr_f64.hip) restating tracking.m:247-300 operation by
 * operation - float64 carrier argument, cos / sin, baseband mix and sums, in a fixed order of additions (bitwise
 * reproducible) - so a closed loop follows the reference's trajectory epoch for epoch instead of statistically.
 * Replay (gc_replay_prepare: GC_E_UNSUPPORTED under GC_PREC_F64) and acquisition are not affected.  A setting of the
 * context; any other value returns GC_E_INVALID. */
enum gc_precision { GC_PREC_F32 = 0, GC_PREC_F64 = 1 };
int gc_set_precision(gc_context* ctx, int precision);
int gc_get_precision(const gc_context* ctx, int* precision);

/* Sampling frequency used for the carrier replica (settings.samplingFreq, tracking.m:280). */
int gc_set_sampling_freq(gc_context* ctx, double fs);

/* Synchronous correlate: `out` receives arms x [I_E,Q_E,I_P,Q_P,I_L,Q_L] doubles per block,
 * blocks in input order, stride = 6*GC_MAX_ARMS doubles per block.
 * Returns GC_E_RANGE (nothing computed) if any block exceeds the IF buffer. */
#define GC_OUT_STRIDE (6 * GC_MAX_ARMS)
int gc_correlate(gc_context* ctx, int nblocks, const gc_block* blocks, double* out);

/* The correlation function of every block at `ntaps` code offsets instead of three (csrc/corr_bank.hip): tap j correlates with the
 * replica ramp ((rem + o_j)*R) : (step*R) : ((((N-1)*step + rem) + o_j)*R), o_j = tap_offsets[j] chips, positive = late
 * (tracking.m:263-270; o = -d, 0, +d are the early, prompt and late ramps bit for bit), carrier and sums as gc_correlate.
 * The padded table of n entries is read PERIODICALLY - index p = ceil(t*m_a), 0-based as in gc_correlate (MATLAB's p + 1), reads entry 1 + mod(p - 1, n - 2) - so
 * offsets of several chips, negative phases and blocks longer than a code period are legal.  el_spacing is ignored.
 * The ramp is MATLAB's colon a : d : b, its end-point rule included: element i is a + i*d below the middle and c - (N-1-i)*d above
 * it, where c = a + (N-1)*d, and c = b only if c - b > -2 eps max(|a|, |b|) - which fails where rem and o_j nearly cancel (rem about
 * a code period, o_j about minus one) and a, b carry the rounding of much larger intermediates.  A descriptor whose colon has N - 1
 * elements for a tap (a + (N-1)*d - b > 2 eps max(|a|, |b|): tracking.m would stop on the size mismatch) is outside this definition;
 * it is not refused, and what is returned for it is not specified.
 * Synchronous, float32 kernels, bitwise reproducible; the library may walk the list in sub-batches of blocks.
 * Accepted: what gc_correlate asks of a descriptor without its three conditions on el_spacing and the table's end, and instead
 *   1 <= ntaps <= GC_BANK_MAX_TAPS, finite offsets (any order, duplicates allowed) with |o_j| * R * m_a < n_a - 2 for every arm,
 *   2^-16 <= code_phase_step * R * max_a(m_a) <= 1 (at most one table entry per sample), every ramp index within int32.
 * GC_E_INVALID also for table_offset != 0 and for a table whose pads are not its period (tab[0] != tab[n-2] or tab[n-1] != tab[1]);
 * GC_E_UNSUPPORTED for a channel with a code window (gc_set_code_window), a step above one entry per sample, and under
 * GC_PREC_F64; GC_E_RANGE / GC_E_STATE as gc_correlate.  Nothing is computed and `out` is not written on any error.
 * out[((b * GC_MAX_ARMS + arm) * ntaps + j) * 2 + {0: I, 1: Q}], unused arms zero. */
#define GC_BANK_MAX_TAPS 64
int gc_correlate_bank(gc_context* ctx, int nblocks, const gc_block* blocks, int ntaps, const double* tap_offsets, double* out);

/* The bank's correlation function at `nfreq` carrier offsets as well: a delay-Doppler map of every block (csrc/corr_bank.hip).
 * Bin m of block b is what gc_correlate_bank returns for the same block with carr_freq replaced by the float64 sum
 * carr_freq + freq_offsets[m] (Hz) - BIT FOR BIT; rem_carr_phase and every other field as they stand, so the carrier phase is
 * referenced to the block's first sample and the bins differ in frequency only.  A result therefore does not depend on which other
 * bins, taps or blocks are in the call.  One kernel computes every table boundary once for a group of bins, where nfreq bank calls
 * repeat the upload, the samples' conversion and the boundary search per bin.
 * Accepted: everything gc_correlate_bank accepts, and 1 <= nfreq <= GC_DDM_MAX_FREQS, finite offsets (any order, duplicates
 * allowed) whose sums with carr_freq are finite.  GC_E_INVALID for nfreq out of range and a non-finite offset or sum; every refusal
 * of the bank (GC_PREC_F64 and code windows: GC_E_UNSUPPORTED) with the bank's status.  Nothing is computed and `out` is not
 * written on any error; an empty block list is GC_OK.
 * out[((((b * GC_MAX_ARMS + arm) * nfreq + m) * ntaps + j) * 2 + {0: I, 1: Q}], unused arms zero. */
#define GC_DDM_MAX_FREQS 64
int gc_correlate_ddm(gc_context* ctx, int nblocks, const gc_block* blocks, int ntaps, const double* tap_offsets, int nfreq,
                     const double* freq_offsets, double* out);

/* Delay-Doppler maps over runs of blocks: gc_correlate_ddm's cells added coherently over each run, then as power over runs
 * (csrc/corr_bank.hip).  Only the maps come back; the per-block cells never leave the device.
 * Block cell: D[b][arm][m][j] is the cell gc_correlate_ddm returns for block b, BIT FOR BIT (the same chunk kernel, the same
 *   chunk-order sum of partials).
 * Runs: the blocks are partitioned in order into nruns runs, run r of run_len[r] >= 1 blocks, the lengths summing to nblocks.  All
 *   blocks of a run name the same channel; first_sample may go in any order inside a run (dn below may be negative, blocks may overlap).
 * Coherent cell of run r, whose first block is b0: the accumulator starts at +0.0 and the blocks are added in block order,
 *     dn = first_sample[b] - first_sample[b0]          (int64, exact as a double)
 *     x  = (freq_offsets[m] * (double)dn) / fs         (one product, one division, each rounded once)
 *     u  = x - rint(x)                                 (exact)
 *     c  = cospi(2u),  s = sinpi(2u)                   (float64)
 *     w  = block_weights ? block_weights[b] : 1.0
 *     re += w * (c * D.re + s * D.im)
 *     im += w * (c * D.im - s * D.re)
 *   every operation rounded by itself (no fused multiply-add): w e^{-i 2 pi f dn / fs} D, the rotation that refers bin m's carrier
 *   phase - which the DDM refers to each block's own first sample - to the run's first block.  Where freq_offsets[m] == 0 the rotation
 *   is exactly 1; a run of one block with weight 1 is D itself.
 * Weights: real and finite; +1 / -1 wipes a data bit or secondary-code chip, 0 drops a block, any other finite value is legal.
 * Power maps: the runs are partitioned in order into nmaps maps, map q of map_len[q] >= 1 runs, the lengths summing to nruns.
 *   pow[q][arm][m][j] starts at +0.0; per run, in run order, p += (re * re + im * im), no fused multiply-add.
 * Outputs: coh[(((r * GC_MAX_ARMS + arm) * nfreq + m) * ntaps + j) * 2 + {0: re, 1: im}],
 *   pow[((q * GC_MAX_ARMS + arm) * nfreq + m) * ntaps + j]; arms the run's channel does not have are zero.  coh may be null (the
 *   coherent sums then never leave the device); pow may be null exactly when nmaps == 0; at least one of the two is asked for.
 * Independence: a cell depends on its own run's blocks only (pow: its own map's) - not on the other runs, taps or bins of the call,
 *   not on the run's position in the list, not on where the library cuts the list into sub-batches.  The same input gives the same
 *   bytes.
 * Refusals: every refusal of gc_correlate_ddm, with its status.  GC_E_INVALID also for nruns < 1 with blocks present, a run_len or
 *   map_len below 1, lengths that do not sum, two channels in one run, a non-finite weight, nmaps < 0, nmaps > 0 with pow null,
 *   nmaps == 0 with coh null.  nblocks == 0 with nruns == 0 and nmaps == 0 is GC_OK (no record needed).  A refused call writes
 *   neither output. */
int gc_correlate_ddm_integrate(gc_context* ctx, int nblocks, const gc_block* blocks, const double* block_weights,
                               int ntaps, const double* tap_offsets, int nfreq, const double* freq_offsets,
                               int nruns, const int32_t* run_len, int nmaps, const int32_t* map_len,
                               double* coh, double* pow);

/* gc_correlate_ddm_integrate under many hypotheses at once, each map's peak picked on the device (csrc/corr_bank.hip): the search
 * over data-bit edges (shifts of the run grid) or over the phases of a secondary code (weight rows) that integrating an untracked
 * channel past one code period needs.  The block cells are computed ONCE, whatever nhyp is.
 * Hypotheses: nused = sum(run_len).  Hypothesis h, 0 <= h < nhyp, looks at the window of nused blocks that starts at block
 *   block_shift[h] (null: every shift 0); its weights are row h of block_weights, laid out [nhyp][nblocks] and indexed by ABSOLUTE
 *   block number (null: every weight 1).
 * Identity: the coherent cells and power maps of hypothesis h are, BIT FOR BIT, what gc_correlate_ddm_integrate returns for
 *     blocks + block_shift[h],  nblocks = nused,  block_weights + h * nblocks + block_shift[h] (or null),
 *   the same taps, bins, run_len and map_len - so the rotation reference b0 is the first block of each run OF THAT HYPOTHESIS.
 * Peaks: peaks[(h * nmaps + q) * GC_MAX_ARMS + arm] is the first maximum of that arm's nfreq x ntaps plane of pow: the cells are
 *   walked bin-major with the tap fastest, starting from cell (0, 0), and the held cell is replaced only on a strict >.  power is
 *   that cell's value, bin and tap its indices.  An arm the run's channel does not have is all zeros: its peak is {0.0, 0, 0}.
 * Outputs: coh[((((h * nruns + r) * GC_MAX_ARMS + arm) * nfreq + m) * ntaps + j) * 2 + {0: re, 1: im}],
 *   pow[(((h * nmaps + q) * GC_MAX_ARMS + arm) * nfreq + m) * ntaps + j], peaks as above.  Each of the three may be null, at least
 *   one is given; pow and peaks need nmaps >= 1.  With peaks alone neither the maps nor the coherent sums leave the device.
 * Independence: a hypothesis's bytes do not depend on which other hypotheses are in the call, on their order, on nhyp, on blocks
 *   outside its window, or on where the library cuts the list.
 * Refusals: every refusal of gc_correlate_ddm_integrate, with its status, checked over the WHOLE block list.  GC_E_INVALID also for
 *   nhyp outside 1 .. GC_DDM_MAX_HYP, a negative shift, block_shift[h] + nused > nblocks, nruns < 1 with blocks present, lengths
 *   that do not sum (map_len to nruns), two channels inside a run of any hypothesis's window, any non-finite entry of
 *   block_weights, peaks or pow given with nmaps == 0, no output at all.  nblocks == 0 with nruns == 0 and nmaps == 0 is GC_OK (no
 *   record needed).  A refused call writes none of its outputs. */
#define GC_DDM_MAX_HYP 128
typedef struct gc_ddm_peak {
  double power;
  int32_t bin;
  int32_t tap;
} gc_ddm_peak;
int gc_correlate_ddm_search(gc_context* ctx, int nblocks, const gc_block* blocks,
                            int nhyp, const int32_t* block_shift, const double* block_weights,
                            int ntaps, const double* tap_offsets, int nfreq, const double* freq_offsets,
                            int nruns, const int32_t* run_len, int nmaps, const int32_t* map_len,
                            double* coh, double* pow, gc_ddm_peak* peaks);

/* Replay (batched, open-loop) mode: descriptors stay resident in HBM so that the timed
 * region contains only kernel work (SURVEY.md §7 hard part 1a). */
int gc_replay_prepare(gc_context* ctx, int64_t nblocks, const gc_block* blocks);
int gc_replay_launch(gc_context* ctx);                 /* asynchronous on the context stream */
int gc_replay_fetch(gc_context* ctx, double* out);     /* waits, copies nblocks*GC_OUT_STRIDE */
/* hipEvent timer on the context stream (bench: roofline.achieved). */
int gc_timer_start(gc_context* ctx);
int gc_timer_stop(gc_context* ctx, double* elapsed_ms);

/* ---- closed-loop tracking (replaces tracking.m:133-368; loop filters on the host) ---- */
enum gc_pll_kind {
  GC_PLL_2ND_ORDER = 0, /* L1CA: tracking.m:308-311 with calcLoopCoef.m:41-45 */
  GC_PLL_3_STATE = 1    /* all other packages: GPS_L5C/include/tracking.m:351-353 */
};

typedef struct gc_track_params {
  double sampling_freq;      /* settings.samplingFreq */
  double code_freq_basis;    /* settings.codeFreqBasis */
  double code_length;        /* settings.codeLength (chips per block) */
  double el_spacing;         /* settings.dllCorrelatorSpacing */
  double int_time;           /* settings.intTime (PDIcode = PDIcarr) */
  double dll_noise_bw, dll_damping;   /* settings.dllNoiseBandwidth, dllDampingRatio */
  double pll_noise_bw, pll_damping;   /* settings.pllNoiseBandwidth, pllDampingRatio */
  int32_t pll_kind;          /* gc_pll_kind */
  int32_t pilot_combine;     /* 0 = data arm only; 1 = combine data+pilot discriminators with the
                                pilot rotated by -pi/2 (GPS_L5C tracking.m:336-348);
                                2 = pilot as is (GAL_E1C tracking.m:303-311,326-331);
                                3 = pilot in quadrature, atan(-I/Q) (BDS/B1C NB_tracking.m:340-342);
                                4 = three arms {data, pilot BOC(1,1), pilot BOC(6,1)} folded into one pilot
                                    p = -sqrt(4/33)*p61 + sqrt(29/33)*(Q11, -I11) (WB_tracking.m:364-369),
                                    which is also what the Pilot_* records then hold (:420-425);
                                5 = the same three arms folded IN PHASE for Galileo E1-C CBOC(6,1,1/11):
                                    p = sqrt(10/11)*p11 - sqrt(1/11)*p61, then as 2 (BASELINE config 3; an extension:
                                    the reference's GAL_E1C package uses the BOC(1,1) replica only) */
  double pf1, pf2, pf3;      /* 3-state filter coefficients (calcLoopCoefCarr.m), if used */
  int64_t skip_samples;      /* settings.skipNumberOfBytes, in samples */
  int32_t n_epochs;          /* codePeriods = settings.msToProcess (tracking.m:90) */
  int32_t table_phase_count; /* API version 2.  0 = off.  GPS L2C: 75 — the pilot arm's table is read through a window
                                that advances by code_length entries per epoch, table_offset[1] = code_length *
                                (phase - 1), phase = channel.CLCodePhase, +1 per epoch, back to 1 after
                                table_phase_count (GPS_L2C/include/tracking.m:261,357-360) */
  /* API version 2: discriminator weights {data, pilot}; all-zero pairs mean 1:1 (the plain averages of L5 / E1).
   * B1C NB: pll 11:29, dll 11:29 (NB_tracking.m:342,349); B1C WB: pll 1:3, dll factor:(1-factor) with
   * factor = CalcWeighingFactor(settings) (WB_tracking.m:382,403). */
  double pll_weight[2];
  double dll_weight[2];
  double dll_scale;          /* both DLL discriminators are multiplied by it: 1 - earlyLateSpc for B1C
                                (NB_tracking.m:346-348); 0 means 1 */
  /* API version 3: C/N0 by the variance-summing method inside the loop (tracking.m:351-358, Common/CNoVSM.m:38-47): after
   * every cno_interval epochs (settings.CNo.VSMinterval; 0 = off) CNoVSM(I_P, Q_P, cno_acc_time) of those epochs' data-arm
   * prompt sums goes to the buffer registered with gc_set_cno_output.  It feeds nothing back into the loop. */
  int32_t cno_interval;
  int32_t cno_mode;          /* gc_cno_mode: which estimator runs every cno_interval epochs */
  double cno_acc_time;       /* settings.CNo.accTime (GC_CNO_VSM) / settings.intTime (GC_CNO_PLD*) */
} gc_track_params;

/* GC_CNO_VSM: Common/CNoVSM.m, one value per interval (trackResults.CNo.VSMValue).
 * GC_CNO_PLD*: BDS/B2a + BDS/B1C Calc_CNo_PLD.m with the bookkeeping of B2a tracking.m:409-432 (cno_interval =
 * settings.CNoInterval): GC_CNO_NPLD values per interval - DataCNo, PilotCNo, B2a_CNo / B1C_CNo (each the 0.5/0.5 average of
 * this interval's estimate with the previous one, zeros before the first) and DataPLD, PilotPLD (the narrow-band lock
 * detectors NBD/NBP with the data bits wiped by sign).  _PILOT_SWAPPED reads the pilot prompt pair as (Q, I)
 * (pilotTRKflag == 1, Calc_CNo_PLD.m:72-75), _PILOT as (I, Q) (pilotTRKflag == 2 of BDS/B1C), plain GC_CNO_PLD has no pilot
 * arm (PilotCNo = PilotPLD = 0, the third value = DataCNo's estimate).  The library evaluates these from the epoch records
 * when the tracking call returns, in every loop mode; they feed nothing back. */
enum gc_cno_mode { GC_CNO_VSM = 0, GC_CNO_PLD = 1, GC_CNO_PLD_PILOT_SWAPPED = 2, GC_CNO_PLD_PILOT = 3 };
#define GC_CNO_NPLD 5

typedef struct gc_channel_init {
  int32_t channel;           /* gc_set_channel index holding this PRN's tables */
  int32_t prn;               /* recorded only */
  double acquired_freq;      /* channel.acquiredFreq, preRun.m:68 */
  double code_freq;          /* initial codeFreq: settings.codeFreqBasis (tracking.m:163) or
                                channel.codeFreq (GPS_L5C tracking.m:165) */
  int64_t code_phase;        /* channel.codePhase, 1-based sample index, preRun.m:69 */
  int32_t table_phase;       /* API version 2: channel.CLCodePhase (1-based; GPS_L2C preRun.m:71), else 0 */
  int32_t reserved;
} gc_channel_init;

/* Per-epoch records, one row of n_epochs doubles per field per channel
 * (trackResults fields, tracking.m:47-86).  Layout: out[(ch*GC_TRK_NFIELDS + field)*n_epochs + e]. */
enum gc_track_field {
  GC_TRK_ABSOLUTE_SAMPLE = 0, GC_TRK_CODE_FREQ, GC_TRK_CARR_FREQ,
  GC_TRK_I_E, GC_TRK_Q_E, GC_TRK_I_P, GC_TRK_Q_P, GC_TRK_I_L, GC_TRK_Q_L,
  GC_TRK_DLL_DISCR, GC_TRK_DLL_DISCR_FILT, GC_TRK_PLL_DISCR, GC_TRK_PLL_DISCR_FILT,
  GC_TRK_REM_CODE_PHASE, GC_TRK_REM_CARR_PHASE,
  GC_TRK_PILOT_I_E, GC_TRK_PILOT_Q_E, GC_TRK_PILOT_I_P, GC_TRK_PILOT_Q_P,
  GC_TRK_PILOT_I_L, GC_TRK_PILOT_Q_L,
  GC_TRK_NFIELDS
};

/* Runs the reference's tracking loop for `nch` channels in lock step: one correlator launch
 * per epoch for all channels, discriminators + loop filters on the host between launches.
 * `epochs_done[ch]` receives the number of completed epochs (== n_epochs unless the IF
 * buffer ran out, in which case the call returns GC_E_RANGE after filling what it could —
 * the reference's early return, tracking.m:241-245).  Under GC_PREC_F64 (gc_set_precision) every epoch is one launch of the
 * float64 kernel for all channels and the host loop reads the sums after a stream synchronise; with gc_track_device the same
 * kernel runs persistently, one workgroup per channel, closing each channel's loop itself (devloop.h): both follow tracking.m
 * epoch for epoch (absoluteSample identical, every other field to ~1e-10 relative on the reference's scenes). */
int gc_track(gc_context* ctx, const gc_track_params* p, int nch, const gc_channel_init* init,
             double* out, int32_t* epochs_done);
/* Where the next tracking calls of this context put trackResults.CNo.VSMValue: cno[ch * (n_epochs / cno_interval) + k] for
 * the k-th completed interval of channel slot ch (caller-owned, `capacity` doubles; NULL unregisters); with a GC_CNO_PLD*
 * mode cno[(ch * (n_epochs / cno_interval) + k) * GC_CNO_NPLD + j].  With the device loop
 * (gc_track_device) the estimator runs in the kernel that closes the loop. */
int gc_set_cno_output(gc_context* ctx, double* cno, int64_t capacity);

/* ---- records larger than the device: tracking window by window ------------------------------------------------------
 * tracking.m reads its file block by block (fread at :226-245) and so handles a record of any length
 * (postProcessing.m:61-96 never loads it whole).  gc_track works on the resident IF buffer; these two entry points carry a
 * channel's loop state from one window of the record to the next. */
typedef struct gc_channel_state {   /* what tracking.m keeps in its local variables between two blocks of a channel */
  int64_t next_sample;       /* first sample of the next block, counted from the start of the RECORD (ftell/dataAdaptCoeff) */
  double code_freq, rem_code_phase;        /* codeFreq, remCodePhase (:219,273) */
  double carr_freq, rem_carr_phase;        /* carrFreq, remCarrPhase (:283,317) */
  double old_code_nco, old_code_error;     /* oldCodeNco, oldCodeError (:326-330) */
  double old_carr_nco, old_carr_error;     /* oldCarrNco, oldCarrError (:308-312) */
  double d_carr_error, d2_carr_error;      /* third-order PLL integrators (GPS_L5C tracking.m:351-353) */
  int32_t table_phase;       /* CLCodePhase (GPS_L2C) */
  int32_t status;            /* 0 running, 2 the record ended inside this channel's next block (tracking.m:241-245) */
  int64_t reserved;
} gc_channel_state;
#define GC_TRACK_RESUME 1        /* `state` holds the end state of the previous window (else it is only written) */
#define GC_TRACK_PAUSE_AT_END 2  /* more of the record follows: stop all channels, in lock step, at the first epoch one of
                                    them cannot read from this window (*paused = 1) instead of ending that channel */
/* gc_track on the window currently in the IF buffer, whose first sample is sample `origin` of the record.  Runs at most
 * p->n_epochs epochs from the given state; `out` / `epochs_done` count from this call's first epoch; absoluteSample is
 * recorded in record coordinates. */
int gc_track_resume(gc_context* ctx, const gc_track_params* p, int nch, const gc_channel_init* init,
                    gc_channel_state* state, int flags, int64_t origin, double* out, int32_t* epochs_done,
                    int32_t* paused);
/* tracking(fid, channel, settings) on a file of any size: the record is read in windows of `window_samples` samples into two
 * device buffers (the next window's read + upload runs while the current one is tracked: at most 2 * window_samples
 * samples are resident), results as gc_track's.  `skip_bytes`: file offset of record sample 0.  Host-closed loop;
 * gc_track_file_device (below) is the same with the loop closed on the device. */
int gc_track_file(gc_context* ctx, const char* path, uint64_t skip_bytes, int dtype, int layout, uint64_t window_samples,
                  const gc_track_params* p, int nch, const gc_channel_init* init, double* out, int32_t* epochs_done);

/* As gc_track, with the loop closed ON THE DEVICE: one persistent cooperative launch runs every
 * epoch; the workgroups sharing a channel exchange self-validating 16-byte {payload, epoch tag} messages (no atomics,
 * no fences) and execute tracking.m:302-335 in float64 themselves (csrc/devloop.h).  Covered: int8 I/Q or Q/I records;
 * single-arm R = 1 channels on the transition-mask kernel (GPS L1 C/A, GLONASS L1OF, BDS B1I) and one- or two-arm
 * channels of any rate and index scale with pilot_combine 0-3 on the lane kernel (GPS L5, BDS B2a / B3I, Galileo E5a /
 * E5b / E1 B+C, BDS B1C narrow-band, GPS L2C with its windowed CL table) in every record format (int8 / int16; I/Q, Q/I,
 * real), and the three-arm folds with a derived third arm on int8 I/Q or Q/I records (Galileo E1-C CBOC, pilot_combine 5;
 * BDS B1C wide-band, pilot_combine 4): every package of the reference (tests/test_gpu_ref_vectors.py).  Other three-arm or
 * mixed-multiplier channels return GC_E_UNSUPPORTED: use gc_track.  Under GC_PREC_F64 every configuration gc_track takes is
 * covered (one float64 workgroup per channel; only a grid that does not fit the device next to other persistent kernels
 * returns GC_E_UNSUPPORTED). */
int gc_track_device(gc_context* ctx, const gc_track_params* p, int nch, const gc_channel_init* init,
                    double* out, int32_t* epochs_done);
/* gc_track_resume with the loop closed on the device: the persistent kernels start every channel from `state` (or, without
 * GC_TRACK_RESUME, from `init`), count positions from `origin` and, with GC_TRACK_PAUSE_AT_END, pause a channel whose next
 * block does not fit the IF buffer instead of ending it.  The channels are NOT in lock step: each pauses at an epoch of its
 * own (epochs_done[c] differ by an epoch or so at a window's end), *paused = 1 when at least one did.  Arguments, flags, `state`
 * and the results' layout are gc_track_resume's - a state written by either function is accepted by the other -, the return
 * codes gc_track_device's (GC_E_UNSUPPORTED exactly where it returns it).  No in-loop C/N0 (gc_set_cno_output) on a window, as
 * with gc_track_resume.  Detect by symbol: GC_API_VERSION is unchanged. */
int gc_track_device_resume(gc_context* ctx, const gc_track_params* p, int nch, const gc_channel_init* init,
                           gc_channel_state* state, int flags, int64_t origin, double* out, int32_t* epochs_done,
                           int32_t* paused);
/* gc_track_file with the loop closed on the device: same windows, reader thread, overlap and first window; one persistent
 * launch per window (gc_track_device_resume).  Results are bit-identical to gc_track_device on the resident record; a file that
 * fits one window goes to gc_track_device.  Where the device loop answers GC_E_UNSUPPORTED the call runs gc_track_file's
 * host-closed windows (gc_debug_last_track_mode tells which loop ran). */
int gc_track_file_device(gc_context* ctx, const char* path, uint64_t skip_bytes, int dtype, int layout, uint64_t window_samples,
                         const gc_track_params* p, int nch, const gc_channel_init* init, double* out, int32_t* epochs_done);

/* ---- several tracking() calls at once (BASELINE config 5: the all-constellation mix) ---------------------------
 * The reference tracks the channels of ONE package per call (tracking.m:133 loops over settings.numberOfChannels with one
 * `settings`); its packages run one after the other.  Channels are independent, so the loops of different packages can
 * run side by side on one GPU - GPS L1 C/A, Galileo E1 and BDS B1C channels on the same L1-band record, L5 / E5a / B2a
 * channels on another - or on several GPUs driven by one host process.  One context per (record, package): own stream,
 * code tables and result buffers; a record loaded into one context is shared with the others by gc_share_if (no copy). */
int gc_share_if(gc_context* dst, gc_context* src);   /* dst reads src's IF record (same device; src must outlive the use) */

typedef struct gc_track_job {
  gc_context* ctx;                /* one job per context */
  const gc_track_params* params;  /* this package's settings */
  const gc_channel_init* init;    /* nch channels, as gc_track */
  double* out;                    /* nch * GC_TRK_NFIELDS * n_epochs doubles, as gc_track */
  int32_t* epochs_done;           /* nch */
  int32_t nch;
  int32_t device_loop;            /* 0: gc_track; 1: gc_track_device, falling back to gc_track where it returns GC_E_UNSUPPORTED */
  int32_t status;                 /* out: the job's return code (GC_E_RANGE = short read, partial records, tracking.m:241-245) */
  int32_t reserved;
  char error[240];                /* out: the job's error text */
} gc_track_job;

/* Runs every job's tracking loop concurrently (one host thread per job for the loop closure, tracking.m:302-335) and
 * returns when all are done: GC_OK, or the first failure (a short read only if nothing worse happened).
 * The jobs' persistent kernels are admitted by a per-device ledger that knows THIS process' kernels only: other processes that
 * run persistent kernels on the same GPU at the same time (several ranks pinned to one device) are invisible to it - serialise
 * their tracking calls (bench.py does, with a file lock) or give every process its own GPU. */
int gc_track_multi(int njobs, gc_track_job* jobs);

/* ---- acquisition (replaces acquisition.m:151-254, resampling off) ------------------- */
typedef struct gc_acq_params {
  double sampling_freq;      /* settings.samplingFreq */
  double code_freq_basis;    /* settings.codeFreqBasis */
  double code_length;        /* settings.codeLength */
  double intermediate_freq;  /* settings.IF */
  double search_band;        /* settings.acqSearchBand (Hz, single-sided) */
  double search_step;        /* settings.acqSearchStep */
  int32_t non_coh_time;      /* settings.acqNonCohTime */
  int32_t source;            /* 0: the IF record (int8 I/Q); GC_ACQ_SOURCE_CONDITIONED: the signal gc_acq_condition left */
  int64_t first_sample;      /* start of longSignal within the IF buffer (or within the conditioned signal) */
  /* API version 3, all optional (0 = the GPS L1 C/A scheme above).  They let the search family whose bins are circular shifts
   * of ONE spectrum (BDS/B1C/include/acquisition.m:137-200) run as a carrier-per-bin search when its transform length cannot be
   * taken by the radix plan - after the input conditioning, where samplesPerCode follows ceil(newFs): circshift(X, k) is the
   * carrier moved by k*fs/N, and the N-point circular correlation with a replica of code_samples samples is the linear one of
   * the block followed by a repeat of its first code_samples samples. */
  int32_t block_len;         /* samples per search block (len10PlusXms, B1C :113); 0: 2*samplesPerCode (acquisition.m:174) */
  int32_t code_samples;      /* samples of each sampled-code row, zeros beyond (samplesXmsLen, B1C :111); 0: samplesPerCode.
                                sigPower is taken over that many samples (B1C :138).  Needs non_coh_time == 1 when set. */
  int32_t n_bins;            /* number of frequency bins; 0: round(2*search_band/search_step) + 1 (acquisition.m:124) */
  int32_t reserved;
  double arm_weight[4];      /* results = sum_arm arm_weight * |ifft(...)| (B1C :186-187: sqrt(11/40), sqrt(29/40)); all 0: 1 */
} gc_acq_params;
#define GC_ACQ_SOURCE_CONDITIONED 1

typedef struct gc_acq_result {
  int32_t coarse_bin;        /* 1-based frequency-bin index, acquisition.m:196 */
  int32_t code_phase;        /* 1-based sample index over 2*samplesPerCode columns, :198 */
  double peak;               /* max(max(results)) */
  double peak_metric;        /* peak/sigPower/acqNonCohTime, :200 */
  double coarse_freq;        /* coarseFreqBin(acqCoarseBin), :169-170 */
} gc_acq_result;

/* ---- acquisition, optional input conditioning (acquisition.m:46-111; the same block with its own
 * bandwidth in ten packages; settings.resamplingflag, off by default): zero-phase band-pass around IF -
 * longSignal = filtfilt(fir1(order, [IF - BW/2, IF + BW/2]*2/fs), 1, longSignal) with filtfilt's 3*order odd-reflected edge
 * samples - then band-pass-sampling decimation by index selection, longSignal(ceil((0:len-1)/newFs*fs)) with the first index
 * forced to 1, newFs = ceil of the centre of the admissible range, and IF -> rem(IF, newFs).  The conditioned complex float
 * signal stays on the device; searches read it with gc_acq_params.source = GC_ACQ_SOURCE_CONDITIONED and the returned
 * sampling frequency / IF (the caller maps code phase and carrier frequency back as acquisition.m:264-276 does). */
typedef struct gc_acq_front_params {
  double sampling_freq;      /* settings.samplingFreq */
  double intermediate_freq;  /* settings.IF */
  double bandwidth;          /* BW (acquisition.m:58: codeFreqBasis*2 + 0.5e6; per-package constants elsewhere) */
  int64_t first_sample;      /* start of longSignal within the IF record */
  int64_t n_samples;         /* length(longSignal) */
  int32_t fir_order;         /* 700 */
  int32_t reserved;
  double band_margin;        /* widening of both normalised band edges: wp = [w1*2/fs - m, w2*2/fs + m]; 0.002 in GPS_L5C / BDS_B2a /
                              * BDS_B1C (GPS_L5C/include/acquisition.m:69), 0 in the other packages (GPS_L1CA :62) */
} gc_acq_front_params;
typedef struct gc_acq_front_result {
  double sampling_freq;      /* settings.samplingFreq after the block (:81) */
  double intermediate_freq;  /* settings.IF after the block (:95) */
  int64_t n_samples;         /* signalLen (:84) */
} gc_acq_front_result;
int gc_acq_condition(gc_context* ctx, const gc_acq_front_params* p, gc_acq_front_result* out);
/* The same device-side signal filled WITHOUT the conditioning block, for what the searches do not read directly (they read int8
 * I/Q records): n samples of the loaded record from first_sample in whatever format it has - int16 files (postProcessing.m:61-96,
 * settings.dataType), Q/I order, real samples - or the caller's own complex samples (re, im interleaved floats;
 * acquisition(longSignal, settings) accepts any complex row).  Then source = GC_ACQ_SOURCE_CONDITIONED and first_sample counts
 * from the signal's start.  gc_acq_condition itself takes the record in any format. */
int gc_acq_signal_from_record(gc_context* ctx, int64_t first_sample, int64_t n);
int gc_acq_set_signal(gc_context* ctx, const float* iq, int64_t n);
/* test hook: the conditioned signal back as n complex floats (re, im interleaved) */
int gc_acq_conditioned(gc_context* ctx, int64_t first, int64_t n, float* dst);

/* `sampled_codes`: nprn rows of samplesPerCode int8 (makeCaTable.m:59-67 output).
 * For each PRN returns the coarse peak (acquisition.m:158-200). */
int gc_acquire_coarse(gc_context* ctx, const gc_acq_params* p, int nprn,
                      const int8_t* sampled_codes, gc_acq_result* out);

/* Data + pilot search: `narms` sampled codes per PRN (row prn*narms + arm); the per-arm correlation
 * magnitudes are added before the non-coherent sum (GPS_L5C/include/acquisition.m:175-216).
 * The PRNs are searched on two lanes; both run on a pair of streams the library keeps per DEVICE for the whole process (forked from and
 * joined into the context's stream inside the call - the call is synchronous as before).  Searches of two contexts on one device at
 * the same time therefore share that pair: correct, and no faster than one after the other. */
int gc_acquire_coarse_multi(gc_context* ctx, const gc_acq_params* p, int nprn, int narms,
                            const int8_t* sampled_codes, gc_acq_result* out);

/* The same with a centre frequency per row: row ip is searched around p->intermediate_freq + freq_offset[ip] (Hz).  One code on
 * several carriers is GLONASS' FDMA search - GLO/GLO_GL1/include/acquisition.m:146-147 runs the L1 C/A scheme once per frequency
 * number K around IF - freqSpacing*K with the common 511-chip code - here as ONE call with the code repeated per row: the rows share
 * the signal spectra (an offset is a whole-bin shift of them) and run on the two PRN lanes.  Every offset must be a whole number of
 * the search's FFT bins, sampling_freq / N, and the bin spacing a whole (or q / den) number of bins - GC_E_UNSUPPORTED otherwise (the
 * caller then searches row by row).  freq_offset == NULL: gc_acquire_coarse_multi.  out[ip].coarse_freq includes the row's offset. */
int gc_acquire_coarse_offsets(gc_context* ctx, const gc_acq_params* p, int nprn, int narms,
                              const int8_t* sampled_codes, const double* freq_offset, gc_acq_result* out);

/* Fine-frequency stage of GPS L1 C/A (acquisition.m:213-254) for one detected PRN:
 * `code` = 1023 chips (+-1), `code_phase` / `coarse_freq` from gc_acquire_coarse.
 * Returns the fine carrier frequency (with the "0 -> 1 Hz" rule of :258-260 applied). */
int gc_acquire_fine_l1ca(gc_context* ctx, const gc_acq_params* p, const int8_t* code,
                         int code_phase, double coarse_freq, double* carr_freq);
/* The same for `ndet` detections in one launch and one read-back (the loop over the detected PRNs of
 * acquisition.m:206-260): codes = ndet rows of code_length chips. */
int gc_acquire_fine_l1ca_batch(gc_context* ctx, const gc_acq_params* p, int ndet, const int8_t* codes,
                               const int32_t* code_phase, const double* coarse_freq, double* carr_freq);

/* ---- acquisition, generic fine-frequency stage (acquisition.m:206-260 and its per-package variants: GPS_L5C
 * :228-252 Neuman-Hofman search, GAL_E5a 100-code secondary search, BDS/B2a non-coherent data+pilot, ...).
 * out[(bin*ncodes + c)*2 + {0,1}] = sum over code period c of x[n] * code[floor(ts*(n + index_offset)/tc) mod
 * code_len] * exp(-1i*2*pi*f_bin*n/fs), n counted from first_sample, f_bin = f0 - bin*fstep.  The hypothesis
 * search over the per-code sums stays with the caller. */
typedef struct gc_fine_params {
  double sampling_freq;      /* settings.samplingFreq */
  double code_freq;          /* settings.codeFreqBasis (tc = 1/code_freq); 0: `code` is a replica already sampled at the
                                sampling rate, one entry per sample - index (n + index_offset) mod code_len (GLONASS' sampled
                                40-code replica, GLO_GL1 acquisition.m:159-164; BDS B1C's table, acquisition.m:236-250; the CL
                                windows of GPS_L2C acquisition.m:140-163) */
  double f0, fstep;          /* FineFreqBins(k) = f0 - fstep*(k-1) */
  int64_t first_sample;      /* absolute index of longSignal(codePhase) */
  int32_t spc;               /* samplesPerCode */
  int32_t ncodes;            /* code periods (40 L1CA, 20 L5/B2a, 100 E5a) */
  int32_t nbins;
  int32_t code_len;          /* settings.codeLength */
  int32_t index_offset;      /* 0: codeValueIndex over (0:K*spc-1) (L1CA :210); 1: over (1:K*spc) (L5 :231); negative:
                                GC_E_INVALID (the index would fall in front of the table) */
  int32_t source;            /* as gc_acq_params.source */
  double dc_re, dc_im;       /* subtracted from every sample first: sig - mean(sig), GPS_L2C acquisition.m:144 (0: nothing) */
} gc_fine_params;

/* mean(x) and var(x) (MATLAB's: normalised by n - 1, of a complex vector) of the n samples from first_sample of the IF record
 * or the conditioned signal (`source` as in gc_acq_params): sigPower = sqrt(var * n) of BDS/B1C acquisition.m:138, the mean
 * of GPS_L2C acquisition.m:144.  The int8 record: exact integer sums, the mean one division of them, the variance the integer
 * n*sum|x|^2 - |sum x|^2 divided once by n*(n - 1) - a few ulp whatever the DC (the searches' sigPower is formed the same way).
 * The conditioned signal: float64 sums in a fixed order, the variance from a second pass over the distances from the mean. */
int gc_acq_signal_stats(gc_context* ctx, int64_t first_sample, int64_t n, int32_t source, double* mean_re, double* mean_im,
                        double* var);

int gc_acquire_fine_sums(gc_context* ctx, const gc_fine_params* p, const int8_t* code, double* out);
/* `ndet` detections per call: detection d uses codes + d*code_len, first_sample[d] and f0[d] instead of the fields of
 * `p`; out[((d*nbins + bin)*ncodes + c)*2 + {0,1}]. */
int gc_acquire_fine_sums_batch(gc_context* ctx, const gc_fine_params* p, int ndet, const int8_t* codes,
                               const int64_t* first_sample, const double* f0, double* out);

/* ---- acquisition, circshift search family (replaces GPS_L2C/include/acquisition.m:40-75,
 * BDS/B1I/include/acquisition.m:76-123, BDS/B1C/include/acquisition.m:137-170): the signal block(s) are mixed with
 * n_carriers carriers and transformed once (gc_acq_shift_prepare); per PRN every Doppler bin is a circular shift of
 * that spectrum by 0 .. n_bins-1 positions before the product with the code spectrum and the inverse transform
 * (gc_acq_shift_search).  Rows are ordered ((carrier * n_signals + signal) * n_bins + bin). */
typedef struct gc_acq_shift_params {
  double sampling_freq;      /* settings.samplingFreq */
  double carrier_f0;         /* first wipe-off carrier in Hz: initFreq */
  double carrier_step;       /* carrier i = carrier_f0 + i*carrier_step (B1I: +freqResolution/Nshifts, L2C: minus) */
  int64_t first_sample;      /* signal block k starts at first_sample + k*n */
  int32_t n;                 /* samplesPerBlock = the reference's transform length; any value: lengths other than 2^a 3^b 5^c run one
                                carrier per row on a longer transform, same rows and results */
  int32_t n_signals;         /* consecutive signal blocks (B1I: signal1, signal2) */
  int32_t n_carriers;        /* Nshifts */
  int32_t n_bins;            /* numberOfFrqBins: circshift(IQfreqDom, bin), bin = 0 .. n_bins-1 */
  int32_t n_arms_max;        /* code components per PRN that gc_acq_shift_search will be given (1..4) */
  int32_t source;            /* as gc_acq_params.source */
} gc_acq_shift_params;

int gc_acq_shift_prepare(gc_context* ctx, const gc_acq_shift_params* p);
/* codes: int8 [narms][n], the local replica already sampled and zero-padded to n by the caller
 * ([cmCodesTable(1:spc) zeros], acquisition.m:44-45).  results(row, :) = sum_arm weight_arm * abs(ifft(shifted
 * spectrum .* conj(fft(code_arm)))) (weights: NULL = 1; B1C sqrt(11/40), sqrt(29/40), acquisition.m:186-187).
 * Returns each row's maximum and its 0-based first position; the rows stay on the device for gc_acq_shift_row. */
int gc_acq_shift_search(gc_context* ctx, int narms, const int8_t* codes, const double* arm_weight,
                        float* row_max, int32_t* row_argmax);
int gc_acq_shift_row(gc_context* ctx, int row, float* out /* n floats */);  /* a row of the last gc_acq_shift_search (GC_E_STATE after a batch call) */
/* A package's whole search in ONE call (replaces the PRN loops BDS/B1I/include/acquisition.m:76-176, GPS/GPS_L2C/include/
 * acquisition.m:40-118, BDS/B1C/include/acquisition.m:170-235 up to the threshold test): codes int8 [nprn][narms][n] go up once, every
 * PRN's transforms are queued back to back, the row maxima of all PRNs come back in one copy, the package's selection rule picks each
 * PRN's row, and - rules with a second peak - the winning rows are transformed again and reduced on the device to
 * {first maximum, second peak}: two read-backs per search instead of two per PRN, no row of n floats crosses the bus.
 *   GC_SHIFT_PICK_GLOBAL            row of the largest row maximum, first column holding it (B1C :193-197); no second peak
 *   GC_SHIFT_PICK_SEQUENTIAL        the sequential rule over (carrier, bin) of GPS_L2C :46-66 (n_signals == 1)
 *   GC_SHIFT_PICK_SEQUENTIAL_PAIRS  the same over the larger of the two signal blocks' maxima, BDS/B1I :87-122 (n_signals == 2)
 * codes: sample_index == NULL: int8 [nprn][narms][n], the local replicas sampled and zero-padded by the caller as for
 * gc_acq_shift_search (code_len, n_index ignored).  Otherwise int8 [nprn][narms][code_len] chip tables and ONE 0-based index vector
 * for all of them: replica(k) = chips(sample_index[k]) for k < n_index, 0 for n_index <= k < n - the make*Table.m gather
 * (ceil(ts*k/tc) depends on the rates only: makeCaTableDMA.m, makeCMTable.m, makeDataTable.m) and the [table zeros] padding done on
 * the device: a few KB per code cross the bus instead of n bytes.
 * second_peak: the largest value among the row's first `period` samples at least `exclude` samples away from the peak, with the
 * reference's three range cases (B1I :141-156, L2C :77-91).  Block lengths without specialised pass kernels (16.368-Msps front ends:
 * padded transforms) run PRN after PRN inside the call, every PRN's rows picked - and guarded in float64, gc_acq_guard_stats - from the
 * written sums (API version 4; version 3 answered GC_E_UNSUPPORTED there).  GC_E_NOMEM: the whole list's buffers do not fit - search
 * PRN by PRN with gc_acq_shift_search / gc_acq_shift_row (float32 rows, the rules and no guard on the caller's side). */
enum { GC_SHIFT_PICK_GLOBAL = 0, GC_SHIFT_PICK_SEQUENTIAL = 1, GC_SHIFT_PICK_SEQUENTIAL_PAIRS = 2 };
typedef struct gc_acq_shift_pick {
  int32_t row;          /* winning row, -1: no value above 0 (the reference leaves the PRN's results at 0) */
  int32_t code_phase;   /* 0-based position of the row's first maximum */
  double peak;          /* its value - float64: the winning cell evaluated again as a float64 correlation (gc_acq_guard_stats) */
  double second_peak;   /* likewise; 0 with GC_SHIFT_PICK_GLOBAL */
} gc_acq_shift_pick;
int gc_acq_shift_search_batch(gc_context* ctx, int nprn, int narms, const int8_t* codes, int code_len, const int32_t* sample_index,
                              int n_index, const double* arm_weight, int rule, int exclude, int period, gc_acq_shift_pick* out /* [nprn] */);
/* What the prepared search writes: samples per row (n), rows of gc_acq_shift_search's outputs (n_carriers * n_signals *
 * n_bins) and the largest narms it takes - for callers that size their buffers (the MEX gateway); any pointer may be NULL. */
int gc_acq_shift_dims(gc_context* ctx, int32_t* n, int32_t* rows, int32_t* n_arms_max);

/* ---- bit synchronisation front end of navigation decoding ------------------------------
 * What every package's NAVdecoding.m does first with a channel's prompt in-phase stream: hard-limit it and cross-correlate it
 * with the sync pattern stretched to the stream's rate - GPS_L1CA/include/NAVdecoding.m:69-85 (160-sample TLM preamble),
 * GAL_E1C :79-88, GAL_E5a :69-95, GAL_E5b :80-100, BDS/B1I :71-105, BDS/B3I :72-97, GLO_GL1 :69-86.
 * out[l] = sum_k s(I_P[l+k]) * pattern[k] for lags l = 0 .. n-1 - the non-negative-lag half of xcorr(bits, pattern),
 * tlmXcorrResult(xcorrLength : 2*xcorrLength - 1) - with s(x) = +1 for x > 0 and -1 otherwise, or with
 * GC_SYNC_ZERO_IS_PLUS +1 for x >= 0 (Galileo E1: bits = (I_P < 0), GAL_E1C/include/NAVdecoding.m:84-85).
 * pattern: m <= 8192 values in {-1, 0, +1}.  The packages' thresholds, spacing rules and word checks (GPS :94-145 ...)
 * stay with the caller (nav_sync.py).  gc_preamble_xcorr is gc_sync_xcorr with flags = 0. */
#define GC_SYNC_ZERO_IS_PLUS 1
int gc_sync_xcorr(gc_context* ctx, const double* i_p, int64_t n, const int8_t* pattern, int m, int flags, float* out);
int gc_preamble_xcorr(gc_context* ctx, const double* i_p, int64_t n, const int8_t* pattern, int m, float* out);

/* Test hook (host only, no GPU): first sample i in [0, n) whose ramp value a + i*step is within eps chips of
 * an integer, or -1 — the exact near-tie analysis that lets the kernels skip their per-chunk filters. */
long long gc_debug_first_sample_near_edge(double a, double step, long long n, double eps);

/* Test hook (host only, no GPU): 1 if the padded table `t6` (n6 entries, read at six times the ramp rate) is the padded
 * table `t1` (n1 entries) with the sign pattern t6[k] = t1[(k + 5) / 6] * (-1)^((k + 5) / 6 + k) - BOC(6,1) next to
 * BOC(1,1) - which lets the lane kernel derive that arm instead of staging its table; 0 otherwise. */
int gc_debug_tables_derivable(const int8_t* t1, int n1, const int8_t* t6, int n6);

/* Test hook: which correlator kernel the last gc_correlate / gc_replay_launch / gc_track / gc_track_device launch used:
 * 0 lane kernel (any chipping rate), 1 fast kernel with one-wave workgroups (float2 tables), 2 fast kernel with
 * four-wave workgroups and int8-pair tables, 3 the same with plain float tables, -1 exact per-sample kernel
 * (mixed ramp multipliers), 6 the float64 per-sample kernel (GC_PREC_F64, gc_correlate and the host-closed loop);
 * -2 before the first launch.  Lets the parity tests prove which path they covered. */
int gc_debug_last_kernel(const gc_context* ctx);

/* Test hook: how the last gc_track / gc_track_device call on this context ran its loop: 0 a correlator launch per epoch,
 * 1 the persistent host-fed kernel, 2 the device loop; -1 before the first call.  A persistent kernel needs all its workgroups
 * resident: a grid that does not fit the device (many channels), or does not fit it together with other contexts' persistent
 * kernels in flight (gc_track_multi), is retried with half as many workgroups per channel until it fits; only a grid that no
 * team size brings under the limit runs with a launch per epoch instead (same records). */
int gc_debug_last_track_mode(const gc_context* ctx);

/* Test hook: how many workgroups shared one block of one channel in the last gc_track / gc_track_device call on this context:
 * the members of a team of the device loop or of the persistent host-fed kernel - after any halving that made the grid fit -
 * or the splits of a launch per epoch; 1 for the float64 loops; 0 before the first call.  Team sizes follow from the channel
 * count, the block length and the device's compute units, so a test can prove which ones it covered. */
int gc_debug_last_track_team(const gc_context* ctx);
/* Test hook for the lane kernel's flush (csrc/corr_common.h: wave_transpose_sum): `k` (1..32) vectors of 64 floats, in[v * 64 + lane];
 * out[v] = the sum over the 64 lanes as the one-wave transposing reduction forms it (the tree's own order of additions). */
int gc_debug_wave_transpose_sum(gc_context* ctx, int k, const float* in, float* out);

/* Test hook: the library's four-step mixed-radix FFT on `nbatch` host sequences of n complex64
 * values (n of the form 2^a 3^b 5^c); output in natural order, unnormalised. */
int gc_debug_fft(gc_context* ctx, int n, int nbatch, const float* in, float* out, int inverse);
/* Test hook (host code only, no context): the plan of an n-point transform - n = n1 x n2, the radices of the columns pass (vectors of
 * n1, element stride n2) and of the rows pass (vectors of n2) in stage order (at most 12 each) and the two passes' tile widths (vectors
 * per workgroup).  GC_E_UNSUPPORTED: no plan for this length (a prime factor above 5, or n2 > 2048). */
int gc_debug_fft_plan(int n, int* n1, int* n2, int* rad1, int* nrad1, int* rad2, int* nrad2, int* cols1, int* cols2);
/* Test hook: gc_acquire_coarse_multi for ONE PRN (codes: int8 [narms][code samples]), then that PRN's whole float32 search surface -
 * the PRN searched again the way the float64 guard's slow path does it, every bin's sums written - as out[bin * n + lag].  *nbins, *n:
 * the search's bins and transform points (a padded transform has more points than the block; only the block's lags count).
 * GC_E_RANGE with both sizes set, before anything is searched, when out_cap (floats) is less than nbins * n. */
int gc_debug_acq_surface(gc_context* ctx, const gc_acq_params* p, int narms, const int8_t* codes, float* out, int64_t out_cap, int32_t* nbins,
                         int32_t* n);

/* The float64 guard of the last search of this context (gc_acquire_coarse*, gc_acq_shift_search_batch): the searches transform in
 * float32, the reference decides in float64 (acquisition.m:196-206 max(max(results)), peakMetric > acqThreshold; BDS/B1I acquisition.m:
 * 141-166 max_peak / second).  Every PRN's winning cell is evaluated again in float64 as a circular correlation at one lag, so peak
 * and peak_metric leave the library without the transforms' rounding; a PRN whose runner-up lies within *eps (relative) of its winner
 * has every cell that close re-evaluated and the reference's first-occurrence rule applied to the float64 values.
 * Three cases keep a float32 decision (the values returned are still the float64 values of the cells named): more than 64 rows of a
 * circshift search within *eps of the chosen one (the float32 choice of the row stands), one of such tied rows with more than 4096
 * cells within *eps of its maximum (that row competes with its float32 maximum), and more than 4096 cells of the chosen row within *eps
 * of its first maximum or second peak (the float32 first maximum and second peak stand) - plateaus, as a record of zeros gives.
 * ties: PRNs of the last search resolved that way; max_dev: largest |float32 peak - float64 peak| / float64 peak over its PRNs. */
int gc_acq_guard_stats(gc_context* ctx, int32_t* ties, double* max_dev, double* eps);

/* ---- a look at the record before acquisition: probeData.m on the device ---------------------------------------------------------
 * What every package's init.m runs first (include/probeData.m:76 the stretch of record, :104 the samples, :128-131 pwelch(data,
 * 32768, 2048, 32768, fs), :146-163 hist(real(data), -128:128), hist(imag(data), -128:128) and dmax): the Welch spectrum and the
 * level histograms of a stretch of the context's IF record, in any of its six formats.  Both calls are synchronous and run on the
 * context's stream; they own their buffers (released by gc_destroy) and leave the acquisition's, the conditioned signal's and the
 * bank's untouched.  New entry points are detected by symbol: GC_API_VERSION is unchanged.
 *
 * Samples are taken in FILE order, as probeData.m:104 does in every package: of a two-component record component 0 is the first
 * value of each pair and component 1 the second, z = c0 + i*c1, whatever the context's layout says (a GC_QI context gives the
 * bytes of a GC_IQ context on the same buffer); of a real record z = c0 and component 1 is absent.
 *
 * gc_probe_psd: pwelch without detrending, two-sided, density scaling, for nspans consecutive spans of nsamples samples each.
 *   step = nfft - noverlap; K = floor((nsamples - noverlap) / step) segments per span, segment k = samples [k*step, k*step + nfft)
 *   of the span, what is left over is dropped (*nsegments = K).
 *   w[n] = 0.54 - 0.46 cos(2 pi n / (nfft - 1)) (GC_WIN_HAMMING: MATLAB's symmetric hamming(nfft)) or 1 (GC_WIN_RECT), applied as
 *   (float)w[n] * (float)x.
 *   psd[s][b] = sum_k |FFT(w .* x_k)[b]|^2 / (K * fs * sum_n w[n]^2), b in FFT order (bin 0 = DC), fs from gc_set_sampling_freq,
 *   sum w^2 in float64.
 * The transform is the acquisition's float32 transform (nfft = 2^a 3^b 5^c, its second factor at most 2048); |X|^2 is added over
 * the segments in float64, in segment order, one accumulator per (span, bin), without atomics: the same input gives the same bytes,
 * and row s of a call with spans is bit for bit the call with nspans = 1 at that span's start - it depends neither on the other
 * spans nor on where the library cuts the segment list into tiles.  A real record gets the two-sided spectrum too; folding it to
 * one side (doubling bins 1 .. nfft/2 - 1) is the caller's.
 *
 * gc_probe_histogram: counts[c][v + 128] = samples of component c with value v, values below -128 or above +128 (int16 records)
 * counted in the end bins - hist(x, -128:128); row 1 is all zero for a real record.  *max_norm2 = max(c0^2 + c1^2) as an exact
 * integer (probeData.m:148 dmax = sqrt(.) + 1 is the caller's).  Integer arithmetic throughout, exact for any range of the record.
 *
 * Refusals (nothing is computed, no output is written): GC_E_INVALID for a null ctx / p / psd / counts, first_sample < 0,
 * nsamples < 1, nspans < 1, nfft < 2, noverlap outside [0, nfft), nsamples < nfft, an unknown window; GC_E_STATE without a record
 * and, for the spectrum, without a sampling frequency; GC_E_UNSUPPORTED for an nfft the transform has no plan for (a prime factor of
 * 7 or more, a row longer than 2048); GC_E_RANGE when a span or the range ends beyond the record; GC_E_NOMEM. */
enum gc_probe_window { GC_WIN_RECT = 0, GC_WIN_HAMMING = 1 };
typedef struct gc_probe_psd_params {
  int64_t first_sample;  /* 0-based sample (pair) index of span 0 */
  int64_t nsamples;      /* samples of EACH span */
  int32_t nfft;          /* segment = window = transform length */
  int32_t noverlap;      /* 0 <= noverlap < nfft */
  int32_t window;        /* gc_probe_window */
  int32_t nspans;        /* >= 1 consecutive spans: span s starts at first_sample + s*nsamples */
} gc_probe_psd_params;   /* 32 bytes */
int gc_probe_psd(gc_context* ctx, const gc_probe_psd_params* p, double* psd /* [nspans][nfft] */, int64_t* nsegments /* may be NULL */);
#define GC_PROBE_HIST_BINS 257
int gc_probe_histogram(gc_context* ctx, int64_t first_sample, int64_t nsamples, uint64_t* counts /* [2][GC_PROBE_HIST_BINS] */,
                       int64_t* max_norm2 /* may be NULL */);
/* Test hook (host code only, no context): segments of an nfft-point gc_probe_psd the library transforms at a time (a tile of its
 * segment list); 0 for nfft < 2. */
long long gc_debug_probe_tile_segments(int nfft);

/* ---- what lies under a tracked signal: the tracked components taken out of a record ------------------------------------------------
 * gc_cancel rebuilds the component every block descriptor describes - the prompt replica of tracking.m:247-300 with the amplitude the
 * record itself gives it - and subtracts it sample by sample (csrc/cancel.hip); the bank, the maps, acquisition and tracking then run
 * on the residual: a reflection under the direct signal's triangle, a weak satellite under a strong one's cross-correlation floor,
 * the direct signal's leak into a down-looking record.  `src` holds the record, the channels and the sampling frequency; `dst` a
 * record of the same sample count, dtype and layout on the same device (gc_alloc_if) that receives the result; dst == src (or a
 * context sharing src's record) works in place and gives the same bytes as out of place.  Synchronous, on src's stream.  New entry
 * points are detected by symbol: GC_API_VERSION is unchanged.
 *
 * Definition, in float64, every operation rounded by itself (no fused multiply-add); the replica is the GC_PREC_F64 correlator's
 * prompt tap (csrc/corr_f64.hip).  Block b (channel ch of R = index_scale and arms a with m_a = arm_mult; N = blksize,
 * s0 = first_sample, rem = rem_code_phase, step = code_phase_step) covers the record samples s0 + i, 0 <= i < N:
 *   carrier   trig_i = ((carr_freq * 2.0) * pi) * (i / fs) + rem_carr_phase,  (sn, cs) = sincos(trig_i)
 *   code      t_i = element i of the reference's colon (rem*R) : (step*R) : (((N-1)*step + rem)*R) - (rem*R) + i*(step*R) below the
 *             middle, the end - (N-1-i)*(step*R) above it, the mean of both ends in the middle;
 *             k = ceil(t_i * m_a) + table_offset[a] clamped to the table, c_a(i) = table_a[k] (code windows, derived arms: the table)
 *   sample    (re, im) of the record: I/Q as stored, Q/I swapped, real records im = 0
 *   baseband  ib = cs*re + sn*im,  qb = cs*im - sn*re
 *   amplitude A[b][a] = amp_in[b][a] where amp_in is given; else the projection A = P / E per component, P = sum_i c_a(i) (ib + j qb)
 *             a float64 sum in a fixed order (bitwise the same from run to run and whatever else is in the call), E = sum_i c_a(i)^2
 *             an exact integer, A = 0 where E == 0.  Arms are projected independently; P is taken from src's record as it is when
 *             the call starts.
 *   model     m_b(i) = sum over a, from +0.0 in arm order, of c_a(i) * ((A_r*cs - A_i*sn) + j (A_r*sn + A_i*cs)); on GC_REAL records
 *             2 * Re(.) - a real record holds half of the phasor.  M[n] = the sum of m_b over the blocks that cover sample n, added
 *             in ascending channel index, starting from +0.0.
 *   output    into dst's record, same position and format: GC_CANCEL_SUBTRACT clamp(rint(x[n] - M[n])), GC_CANCEL_MODEL
 *             clamp(rint(M[n])) per component; rint rounds to even, the clamp is the dtype's full range.  A sample no block covers is
 *             copied (SUBTRACT) or zero (MODEL).
 * amp_out (may be NULL) receives the amplitudes used, [nblocks][GC_MAX_ARMS][2] = {re, im} in the caller's block order as amp_in,
 * arms the block's channel does not have zero.
 * Independence: a sample's output depends on its own input sample and on the blocks that cover it - not on the list's order beyond
 * the rule above, not on the other blocks of the call.  The same input gives the same bytes.  The context's precision setting is
 * ignored: float64 always.
 * Accepted: what gc_correlate asks of a descriptor with el_spacing ignored (taken as 0); the blocks in any order; at most
 * GC_CANCEL_MAX_CHANNELS distinct channels per call.  Any finite carr_freq is accepted, but where carr_freq * 2.0 or its product
 * with pi leaves the float64 range (|carr_freq| above about 2.8e307) trig_i is infinite or NaN and the output of the samples the
 * block covers, and its projected amplitude, are unspecified (the call still returns GC_OK and writes inside the record only).  GC_E_INVALID for two blocks of one channel that overlap, a dst record that
 * differs from src's in device, sample count, dtype or layout (or overlaps it without being it), an unknown mode, a non-finite amp_in
 * of an arm the block's channel has, null src, dst, or blocks with nblocks > 0; GC_E_RANGE / GC_E_STATE as gc_correlate (GC_E_STATE
 * also for a dst without a record).  A refused call writes nothing.  nblocks == 0 is GC_OK: a plain copy (SUBTRACT) or zeros (MODEL). */
#define GC_CANCEL_MAX_CHANNELS 64
enum gc_cancel_mode { GC_CANCEL_SUBTRACT = 0, GC_CANCEL_MODEL = 1 };
int gc_cancel(gc_context* src, gc_context* dst, int nblocks, const gc_block* blocks,
              const double* amp_in  /* [nblocks][GC_MAX_ARMS][2] or NULL */,
              double* amp_out       /* same layout, or NULL */, int mode);

/* ---- interference the receiver does not know: pulses blanked in a record ---------------------------------------------------------
 * What gc_probe_histogram shows far out of the level histogram - DME / TACAN pulse pairs in the band of GPS L5, Galileo E5a / E5b
 * and BDS B2a, radar, bursts of a neighbouring service - is blanked where the record lives (csrc/excise.hip); acquisition, tracking,
 * the bank and the maps then run on the cleaned record.  The records are gc_cancel's: `src` holds the record, `dst` is a context on
 * the same device whose record has the same sample count, dtype and layout (gc_alloc_if); dst == src, or a context sharing src's
 * record, works in place and gives the bytes of the out-of-place call.  Synchronous, on src's stream.  The call owns its buffers
 * (released by gc_destroy) and touches none of the acquisition's, the conditioned signal's, the bank's or the probe's.  New entry
 * points are detected by symbol: GC_API_VERSION is unchanged.
 *
 * Samples are taken in FILE order, as the probe takes them: c0 is the first value of each pair and c1 the second, whatever the
 * context calls its layout; a real record has c0 only.
 *
 * Definition, in exact 64-bit integers (an int16 pair (-32768, -32768) has norm 2^31).  Only the samples of the range
 * [first_sample, first_sample + nsamples) are examined.  Sample h of the range is hot iff c0^2 + c1^2 > threshold2 (real records:
 * c0^2).  A hot sample h blanks [h - before, h + after], cut at the range's ends: sample n of the range is blanked - every one of
 * its components written as 0 - iff a hot sample lies in [n - after, n + before] within the range.  Every other sample of the
 * range keeps its bytes; the samples of the record outside the range are copied when out of place and untouched when in place.
 * stats (may be NULL): hot samples, blanked samples (the hot ones included), maximal runs of consecutive blanked samples and the
 * longest run.  The same input gives the same bytes and the same statistics.
 *
 * Refusals (a refused call writes nothing: not dst, not stats): GC_E_INVALID for a null src / dst / p, first_sample < 0,
 * nsamples < 1, threshold2 < 0, before or after outside [0, GC_EXCISE_MAX_GUARD], a dst record that differs from src's in device,
 * sample count, dtype or layout, or overlaps it without being it; GC_E_STATE for a src or dst without a record; GC_E_RANGE when the
 * range ends beyond the record; GC_E_NOMEM. */
#define GC_EXCISE_MAX_GUARD 4096
typedef struct gc_excise_pulse_params {
  int64_t first_sample;  /* 0-based sample (pair) index of the range */
  int64_t nsamples;      /* samples of the range, >= 1 */
  int64_t threshold2;    /* sample n is hot iff c0^2 + c1^2 > threshold2 */
  int32_t before, after; /* samples blanked in front of and behind a hot sample, 0 .. GC_EXCISE_MAX_GUARD */
} gc_excise_pulse_params;  /* 32 bytes */
typedef struct gc_excise_pulse_stats {
  int64_t hot;      /* hot samples */
  int64_t blanked;  /* samples blanked, hot samples included */
  int64_t runs;     /* maximal runs of blanked samples */
  int64_t longest;  /* longest run */
} gc_excise_pulse_stats;   /* 32 bytes */
int gc_excise_pulses(gc_context* src, gc_context* dst, const gc_excise_pulse_params* p, gc_excise_pulse_stats* stats /* may be NULL */);

/* ---- ... and carriers notched: a gain per frequency bin by weighted overlap-add on the library's own transform -----------------------
 * What gc_probe_psd shows standing over the noise - a CW spur, a narrow-band carrier - is taken out of a range of the record by a
 * gain per bin of an nfft-point transform: bin b of `gain` is bin b of gc_probe_psd (bin 0 = DC, samples in file order z = c0 + i c1,
 * z = c0 for a real record).  The records, the in-place rule, the stream and the buffers are gc_excise_pulses'.
 *
 * Definition.  H = nfft / 2; w[n] = (float) sin(pi (n + 0.5) / nfft), the sine in float64; s[n] = (float)((double)w[n] / nfft).
 * w^2 of the two halves adds to 1: a gain of all ones is the identity.  K = ceil(nsamples / H) + 1 segments; segment k covers the
 * range-relative samples [(k-1) H, (k+1) H), samples outside [0, nsamples) count as zero (zero padding: the record's samples next
 * to the range are not read).  All arithmetic is float32, every operation rounded by itself:
 *   a_k[n] = w[n] * (float)x           X_k = the library's forward transform of a_k (the acquisition's, as gc_probe_psd)
 *   Y_k[b] = gain[b] * X_k[b]          per component
 *   v_k    = the library's unnormalised inverse transform of Y_k
 *   c_k[n] = s[n] * v_k[n]
 *   y[m]   = c_k0[H + m mod H] + c_(k0+1)[m mod H],  k0 = floor(m / H), for range sample m
 * The output is clamp(rint(y)) per component (rint rounds to even, the clamp is the dtype's full range); on real records the
 * imaginary part of y is dropped.  values (may be NULL; host memory, [nsamples][2] = {re, im}) receives y[m] exactly as it was
 * rounded, the imaginary part of a real record's included.  Samples of the record outside the range are copied when out of place
 * and untouched when in place.
 * Guarantees: the same input gives the same bytes.  A sample's output depends on its two segments only - not on where the library
 * cuts the segment list into tiles (gc_debug_excise_tile_segments).  In place equals out of place: where a tile ends, the last
 * segment's contributions are carried, its samples are not read again after they were written.
 *
 * Refusals (a refused call writes nothing: not dst, not values): GC_E_INVALID for a null src / dst / p / gain, first_sample < 0,
 * nsamples < 1, nfft < 4 or odd, reserved != 0, a gain that is not finite, a dst mismatch as above; GC_E_UNSUPPORTED for an nfft
 * the transform has no plan for (a prime factor of 7 or more, a row longer than 2048); GC_E_STATE, GC_E_RANGE, GC_E_NOMEM as above. */
typedef struct gc_excise_bins_params {
  int64_t first_sample;  /* 0-based sample (pair) index of the range */
  int64_t nsamples;      /* samples of the range, >= 1 */
  int32_t nfft;          /* even, >= 4, 2^a 3^b 5^c with a plan */
  int32_t reserved;      /* 0 */
} gc_excise_bins_params;   /* 24 bytes */
int gc_excise_bins(gc_context* src, gc_context* dst, const gc_excise_bins_params* p,
                   const float* gain  /* [nfft] */,
                   float* values      /* [nsamples][2] or NULL */);
/* Test hook (host code only, no context): segments of an nfft-point gc_excise_bins the library transforms at a time (a tile of its
 * segment list); 0 for nfft < 4. */
long long gc_debug_excise_tile_segments(int nfft);

/* ---- ... and swept interference cut cell by cell: a decision per bin in every segment -------------------------------------------------
 * A chirp jammer crosses most of the band many times per millisecond: every bin is hit a small share of the time, the Welch spectrum
 * shows a plateau and no line, and a sample is a few times the noise level - neither a gain per bin nor the blanker takes it out.
 * gc_excise_sweep decides bin by bin in every segment of gc_excise_bins' overlap-add and cuts only the time-frequency cells that
 * stand over a limit.  The records and `dst` (out of place, in place, a context that shares the record), the stream and the buffers,
 * file order, H, K = ceil(nsamples / H) + 1, w, s, the zero padding outside the range, X_k, the inverse transform, c_k, y and the
 * rounding into the record are gc_excise_bins'.  New here, all in float32, every operation rounded by itself (no fused multiply-add):
 *   power   P_k[b] = X_k[b].re * X_k[b].re + X_k[b].im * X_k[b].im
 *   hot     cell (k, b) is hot iff P_k[b] > limit[b]: a limit of +INF protects a bin, a limit of 0 makes it hot wherever P > 0
 *   cut     cell (k, b) is cut iff some bin b' of segment k is hot with min(|b - b'|, nfft - |b - b'|) <= widen: the distance is
 *           circular (bin nfft - 1 is next to bin 0); with 2 widen + 1 >= nfft one hot bin cuts the segment
 *   Y_k[b]  (+0, +0) where cut; elsewhere gain[b] * X_k[b] per component, X_k[b] itself with a NULL gain
 * out (may be NULL; host memory, every member may be NULL): values as gc_excise_bins'; power [K][nfft], P_k[b] as it was compared;
 * hot and cut [K][W] with W = (nfft + 63) / 64 words per segment, bin b bit b & 63 of word [k][b >> 6], the bits from nfft on 0;
 * bin_cut [nfft], the segments in which bin b was cut.  power and the masks are in natural bin order, gc_probe_psd's.
 * stats (may be NULL): K, the hot cells, the cut cells (the hot ones included), the segments with a cut cell, the most cut cells of
 * one segment.  The counts are integer sums: exact, whatever order the device forms them in.
 * Guarantees: the same input gives the same bytes, values, power, masks and counts.  A segment's decisions depend on that segment
 * only - not on the tile of the segment list it falls in (gc_debug_excise_tile_segments), not on which of the optional outputs were
 * asked for.  In place equals out of place.  With every limit at +INF the call is gc_excise_bins with the same gain byte for byte,
 * record and values; a NULL gain is a gain of ones.
 *
 * Refusals (a refused call writes nothing: not dst, not out's arrays, not stats): those of gc_excise_bins (there is no reserved
 * member), and GC_E_INVALID for a null limit, a limit[b] that is NaN or negative, a widen outside [0, GC_EXCISE_MAX_WIDEN] and a gain
 * that is not finite. */
#define GC_EXCISE_MAX_WIDEN 64
typedef struct gc_excise_sweep_params {
  int64_t first_sample;   /* 0-based sample (pair) index of the range */
  int64_t nsamples;       /* >= 1 */
  int32_t nfft;           /* even, >= 4, 2^a 3^b 5^c with a plan */
  int32_t widen;          /* 0 .. GC_EXCISE_MAX_WIDEN */
} gc_excise_sweep_params; /* 24 bytes */
typedef struct gc_excise_sweep_out {   /* host memory, every member may be NULL */
  float*    values;   /* [nsamples][2]: y before rounding, as gc_excise_bins */
  float*    power;    /* [K][nfft]: P_k[b] as it was compared */
  uint64_t* hot;      /* [K][W] */
  uint64_t* cut;      /* [K][W] */
  int64_t*  bin_cut;  /* [nfft]: segments in which bin b was cut */
} gc_excise_sweep_out;
typedef struct gc_excise_sweep_stats {
  int64_t segments;      /* K */
  int64_t hot;           /* hot cells */
  int64_t cut;           /* cut cells, the hot ones included */
  int64_t segments_cut;  /* segments with a cut cell */
  int64_t most_cut;      /* most cut cells in one segment */
} gc_excise_sweep_stats;  /* 40 bytes */
int gc_excise_sweep(gc_context* src, gc_context* dst, const gc_excise_sweep_params* p,
                    const float* limit /* [nfft] */, const float* gain /* [nfft] or NULL */,
                    const gc_excise_sweep_out* out /* may be NULL */,
                    gc_excise_sweep_stats* stats /* may be NULL */);

/* ---- a band of a record as a record at a lower rate: the digital down-converter -----------------------------------------------------
 * gc_downconvert filters a record with a complex FIR, keeps every D-th output, rotates it by a numerically controlled oscillator and
 * requantises it into a SECOND record (csrc/ddc.hip): a 50 Msps L5 file, one FDMA carrier of a GLONASS record, the C/A main lobe of
 * an 18 Msps file become records that every correlator here reads at D times fewer samples.  `src` holds the record (its own, or one
 * shared through gc_share_if) and the sampling frequency; `dst` is another context on the same device with a record from gc_alloc_if
 * or gc_attach_if - any sample count, dtype and layout.  Synchronous, on src's stream.  The call owns its buffers (released by
 * gc_destroy) and touches none of the acquisition's, the probe's, the bank's or the excision's.  New entry points are detected by
 * symbol: GC_API_VERSION is unchanged.
 *
 * Definition, in float64, every operation rounded by itself (no fused multiply-add).  fs = src's gc_set_sampling_freq,
 * D = decim, T = ntaps, g[k] = (gr[k], gi[k]) = taps[k].
 *   input     x[n] = (re, im) of record sample n: I/Q as stored, Q/I swapped, real records im = 0; x[n] = 0 for n < 0 and for
 *             n >= the record's sample count
 *   position  n_m = first_sample + m * D for output m, 0 <= m < noutputs
 *   filter    a_r = a_i = +0.0; for k = 0 .. T-1 in ascending order, with x = x[n_m - k]:
 *               pr = gr[k]*xr - gi[k]*xi,  pi = gr[k]*xi + gi[k]*xr,  a_r = a_r + pr,  a_i = a_i + pi
 *   NCO       exact integers modulo 2^64, addressed by the absolute record index:
 *               phase_step = (uint64)(int64) llrint(ldexp(carr_freq / fs, 64))
 *               phase0: q = carr_phase / 6.283185307179586, r = q - rint(q), X = ldexp(r, 64); 2^63 where X = +-2^63, else
 *                       (uint64)(int64) llrint(X)
 *               ph_m = phase0 + phase_step * (uint64) n_m
 *               ang = (double)(int64) ph_m * (6.283185307179586 * 2^-64), in [-pi, pi]: no large-argument reduction, and the phase
 *                     of a sample does not depend on where a call starts;  (sn, cs) = sincos(ang)
 *   rotation  yr = cs*a_r + sn*a_i,  yi = cs*a_i - sn*a_r
 *   store     into dst's record at sample dst_first + m, in dst's own format: clamp(rint(.)) per component (rint rounds to even, the
 *             clamp is the dtype's full range); (yr, yi) for GC_IQ, (yi, yr) for GC_QI, yr alone for GC_REAL.
 *   result    clipped and sum_sq count what was stored (yi of a real dst is not counted).
 * The taps carry any gain; the library applies none.
 * Guarantees: dst's bytes outside [dst_first, dst_first + noutputs) are untouched.  The same input gives the same bytes and
 * statistics.  An output depends on its own T input samples and on n_m only - not on the tile it falls in (gc_debug_ddc_tile_outputs),
 * not on the call it belongs to: two calls on [n_0, n_0 + a D) and from n_0 + a D on, with dst_first moved by a, write the bytes of
 * the single call.
 *
 * Refusals (a refused call writes nothing: not dst, not res): GC_E_INVALID for a null src / dst / p / taps, first_sample or
 * dst_first < 0, noutputs < 1, decim outside [1, GC_DDC_MAX_DECIM], ntaps outside [1, GC_DDC_MAX_TAPS], a tap, carr_freq or carr_phase
 * that is not finite, |carr_freq| >= fs / 2, a dst on another device, a dst record that is src's or overlaps it; GC_E_STATE for a src
 * or dst without a record and a src without a sampling frequency; GC_E_RANGE when dst_first + noutputs exceeds dst's record, and when
 * the last output has no record sample under it (n_last - (T-1) >= src's sample count); GC_E_NOMEM. */
#define GC_DDC_MAX_TAPS  2048
#define GC_DDC_MAX_DECIM 64
typedef struct gc_ddc_params {
  int64_t first_sample;  /* record index n_0 of output 0's newest input sample, >= 0 */
  int64_t noutputs;      /* >= 1 */
  int64_t dst_first;     /* output m is written to sample dst_first + m of dst's record, >= 0 */
  int32_t decim;         /* D, 1 .. GC_DDC_MAX_DECIM */
  int32_t ntaps;         /* T, 1 .. GC_DDC_MAX_TAPS */
  double  carr_freq;     /* Hz, |carr_freq| < fs / 2 (fs = src's gc_set_sampling_freq) */
  double  carr_phase;    /* radians, the NCO's phase at record sample 0 */
} gc_ddc_params;         /* 48 bytes */
typedef struct gc_ddc_result {
  uint64_t phase_step;   /* NCO increment per INPUT sample, turns * 2^64 */
  uint64_t phase0;       /* NCO phase at record sample 0, turns * 2^64 */
  int64_t  clipped;      /* stored components whose rint(y) lay outside dst's integer range */
  uint64_t sum_sq;       /* exact sum of the squares of the stored components */
  double   carr_freq;    /* the frequency the NCO runs at: (int64) phase_step * 2^-64 * fs */
} gc_ddc_result;         /* 40 bytes */
int gc_downconvert(gc_context* src, gc_context* dst, const gc_ddc_params* p,
                   const double* taps /* [ntaps][2] = {re, im} */, gc_ddc_result* res /* may be NULL */);
/* Test hook (host code only, no context): outputs a workgroup of the kernel takes (a tile); 0 for a decim or ntaps out of range. */
long long gc_debug_ddc_tile_outputs(int decim, int ntaps);

/* ---- a record at a rational multiple of its rate: the polyphase resampler -------------------------------------------------------------
 * gc_resample is gc_downconvert at the rate change L / M (csrc/resample.hip): the record is taken as if L - 1 zeros stood between its
 * samples, filtered with a complex FIR given at the rate fs * L (the prototype), every M-th of those outputs is kept, rotated by the NCO
 * and requantised into a SECOND record at the rate fs * L / M: 18 Msps become 4 or 8 Msps, 50 Msps become 20, the records of two front
 * ends meet at one rate.  Only the taps that meet a record sample are multiplied.  src, dst, the stream, the buffers (its own, released
 * by gc_destroy) and the detection by symbol are gc_downconvert's.
 *
 * Definition, in float64, every operation rounded by itself (no fused multiply-add).  fs = src's gc_set_sampling_freq, L = interp,
 * M = decim, T = ntaps, g[k] = (gr[k], gi[k]) = taps[k]; a TICK is 1 / L of an input sample.
 *   input     x[n] as in gc_downconvert: zero for n < 0 and for n >= the record's sample count
 *   position  u_m = first_tick + m * M for output m, 0 <= m < noutputs;  n_m = u_m div L,  p_m = u_m mod L
 *   filter    a_r = a_i = +0.0; for j = 0, 1, .. in ascending order while k = j * L + p_m < T, with x = x[n_m - j] and g = g[k]:
 *               pr = gr*xr - gi*xi,  pi = gr*xi + gi*xr,  a_r = a_r + pr,  a_i = a_i + pi
 *             The kernel pads the prototype with zero taps up to J * L, J = ceil(T / L), and runs j = 0 .. J-1 for every output: a
 *             zero tap adds +-0 to a sum that started at +0.0, which changes no stored integer and no statistic.
 *   NCO       exact integers modulo 2^64, addressed by the absolute TICK:
 *               phase_step = (uint64)(int64) llrint(ldexp(carr_freq / (fs * (double)L), 64))
 *               phase0 as in gc_downconvert (the NCO's phase at tick 0)
 *               ph_m = phase0 + phase_step * (uint64) u_m
 *   ang, (sn, cs), rotation, store, result: gc_downconvert's, operation for operation.
 *   res->carr_freq = ldexp((double)(int64) phase_step, -64) * (fs * (double)L);  res->out_rate = (fs * (double)L) / (double)M.
 * Guarantees: gc_downconvert's.  dst's bytes outside [dst_first, dst_first + noutputs) are untouched; the same input gives the same
 * bytes and statistics; an output depends on its own samples and on u_m only - not on the tile (gc_debug_rs_tile_outputs), not on the
 * call: two calls on [u_0, u_0 + a M) and from u_0 + a M on, with dst_first moved by a, write the bytes of the single call.  With
 * interp == 1 every byte and every field of the result is gc_downconvert's with first_sample = first_tick and decim = M (out_rate is
 * the one field more).
 *
 * Refusals (a refused call writes nothing): gc_downconvert's, status for status and in its order, with these among the argument
 * checks: GC_E_INVALID for interp outside [1, GC_RS_MAX_INTERP], decim outside [1, GC_DDC_MAX_DECIM * interp], ntaps outside
 * [1, GC_RS_MAX_TAPS] and reserved != 0; |carr_freq| is held against fs / 2; after dst's range, GC_E_INVALID for a last tick
 * first_tick + (noutputs - 1) * M that does not fit in 63 bits; then GC_E_RANGE when the last output has no record sample under it
 * (n_last - (J-1) >= src's sample count). */
#define GC_RS_MAX_INTERP 64
#define GC_RS_MAX_TAPS   2048
typedef struct gc_rs_params {
  int64_t first_tick;    /* u_0 >= 0: position of output 0 in ticks of 1 / L input sample */
  int64_t noutputs;      /* >= 1 */
  int64_t dst_first;     /* output m is written to sample dst_first + m of dst's record, >= 0 */
  int32_t interp;        /* L, 1 .. GC_RS_MAX_INTERP */
  int32_t decim;         /* M, 1 .. GC_DDC_MAX_DECIM * L: the rate falls to no less than 1 / 64 */
  int32_t ntaps;         /* T, 1 .. GC_RS_MAX_TAPS: the prototype at the rate fs * L */
  int32_t reserved;      /* 0 */
  double  carr_freq;     /* Hz, |carr_freq| < fs / 2 */
  double  carr_phase;    /* radians, the NCO's phase at tick 0 */
} gc_rs_params;          /* 56 bytes */
typedef struct gc_rs_result {
  uint64_t phase_step;   /* NCO increment per TICK, turns * 2^64 */
  uint64_t phase0;       /* NCO phase at tick 0, turns * 2^64 */
  int64_t  clipped;      /* stored components whose rint(y) lay outside dst's integer range */
  uint64_t sum_sq;       /* exact sum of the squares of the stored components */
  double   carr_freq;    /* the frequency the NCO runs at */
  double   out_rate;     /* (fs * L) / M, each operation rounded by itself: dst's sampling frequency */
} gc_rs_result;          /* 48 bytes */
int gc_resample(gc_context* src, gc_context* dst, const gc_rs_params* p,
                const double* taps /* [ntaps][2] = {re, im} */, gc_rs_result* res /* may be NULL */);
/* Test hook (host code only, no context): outputs a workgroup of the kernel takes (a tile); 0 for an interp, decim or ntaps out of range. */
long long gc_debug_rs_tile_outputs(int interp, int decim, int ntaps);

/* ---- several antennas, one front end: the records' covariance and their weighted sum -------------------------------------------------
 * gc_array_covariance and gc_array_combine are the two halves of antenna-array null steering that run over every sample (csrc/array.hip):
 * the covariance of K records tells the receiver where wide-band interference comes from, a weighted sum of the records puts a null
 * there.  What lies between them - a K T x K T solve, the power-inversion rule - is host arithmetic (receiver.null_steer,
 * matlab/gnsscorr_null_steer.m).  `srcs` are K contexts on one device whose records share one dtype and layout (the same context may
 * appear twice); `dst` is another context on that device with a record of any sample count, dtype and layout.  Both calls are
 * synchronous, on srcs[0]'s stream, after the pending work of every other source's stream and of dst's; their buffers are srcs[0]'s
 * (released by gc_destroy).  No sampling frequency is needed.  New entry points are detected by symbol: GC_API_VERSION is unchanged.
 *
 * Shared by both calls
 *   x_a[n] = (re, im) of sample n of srcs[a]'s record, as gc_downconvert reads it: I/Q as stored, Q/I swapped, real records im = 0;
 *   x_a[n] = 0 for n < 0.  (No call reads behind a record's end: see the refusals.)
 *
 * gc_array_covariance, exact integers.  K = nrecords, L = nlags:
 *   C[l][a][b] = sum over n = first_sample .. first_sample + nsamples - 1 of x_a[n] * conj(x_b[n - l]),  0 <= l < L,  0 <= a, b < K
 *     re = sum (ar*br + ai*bi),  im = sum (ai*br - ar*bi)        with (ar, ai) = x_a[n], (br, bi) = x_b[n - l]
 *   x_b[n - l] in front of first_sample is the record's own sample; it is zero only in front of sample 0.
 *   cov[((l * K + a) * K + b) * 2 + {0, 1}] = {re, im}.  nsamples <= 2^31 keeps every sum inside 63 bits for int16 records
 *   (2^31 samples * 2 products * 2^30).
 * Guarantees: the same input gives the same numbers; they do not depend on the tile (gc_debug_array_tile_outputs); two calls on adjacent
 * ranges add up to one call on the whole range; lag 0 is Hermitian, C[0][a][b] == conj(C[0][b][a]); C[0][a][a].re is the record's sum
 * of squares over the range.
 *
 * gc_array_combine, in float64, every operation rounded by itself (no fused multiply-add).  K = nrecords, T = ntaps,
 * w[a][k] = (wr, wi) = weights[(a * T + k) * 2 + {0, 1}]:
 *   filter    for output m, 0 <= m < noutputs, with n = first_sample + m:  a_r = a_i = +0.0; for a = 0 .. K-1 in ascending order and,
 *             within each a, k = 0 .. T-1 in ascending order, with x = x_a[n - k]:
 *               pr = wr*xr - wi*xi,  pi = wr*xi + wi*xr,  a_r = a_r + pr,  a_i = a_i + pi
 *   store     (a_r, a_i) into dst's record at sample dst_first + m, as gc_downconvert stores (yr, yi): clamp(rint(.)) per component
 *             in dst's own format.
 *   result    clipped and sum_sq as gc_downconvert counts them.
 * There is no NCO and no decimation (gc_downconvert / gc_resample run on the result).  The weights are applied as given: a caller who
 * wants w^H x conjugates.
 * Guarantees: dst's bytes outside [dst_first, dst_first + noutputs) are untouched.  The same input gives the same bytes and statistics.
 * An output depends on its own K T samples only - not on the tile, not on the call: pieces join to the whole.  With K = 1 every byte
 * and both statistics are gc_downconvert's with decim = 1, carr_freq = 0, carr_phase = 0 and the same taps (its rotation by the exact
 * angle 0 adds +-0, which changes no stored integer).
 *
 * Refusals (a refused call writes nothing: not cov, not dst, not res), in this order: GC_E_INVALID for a null srcs / p / cov / weights /
 * dst or a null entry of srcs, nrecords outside [1, GC_ARRAY_MAX_RECORDS], nlags or ntaps outside [1, GC_ARRAY_MAX_TAPS], first_sample
 * or dst_first < 0, nsamples outside [1, 2^31], noutputs < 1, a weight that is not finite, a source or dst on another device than
 * srcs[0], sources of different dtype or layout, a dst record that is, or overlaps, any source's; GC_E_STATE for a source or dst
 * without a record; GC_E_RANGE when first_sample + nsamples (or + noutputs) exceeds any source's sample count or dst_first + noutputs
 * exceeds dst's; GC_E_NOMEM. */
#define GC_ARRAY_MAX_RECORDS 8
#define GC_ARRAY_MAX_TAPS    32      /* taps of gc_array_combine and lags of gc_array_covariance */
typedef struct gc_array_cov_params {
  int64_t first_sample;  /* >= 0 */
  int64_t nsamples;      /* 1 .. 2^31 */
  int32_t nrecords;      /* K, 1 .. GC_ARRAY_MAX_RECORDS */
  int32_t nlags;         /* L, 1 .. GC_ARRAY_MAX_TAPS: lags 0 .. L-1 */
} gc_array_cov_params;   /* 24 bytes */
int gc_array_covariance(gc_context* const* srcs, const gc_array_cov_params* p, int64_t* cov /* [L][K][K][2] = {re, im} */);
typedef struct gc_array_combine_params {
  int64_t first_sample;  /* record index of output 0's newest input sample, >= 0 */
  int64_t noutputs;      /* >= 1 */
  int64_t dst_first;     /* output m is written to sample dst_first + m of dst's record, >= 0 */
  int32_t nrecords;      /* K, 1 .. GC_ARRAY_MAX_RECORDS */
  int32_t ntaps;         /* T, 1 .. GC_ARRAY_MAX_TAPS */
} gc_array_combine_params;  /* 32 bytes */
typedef struct gc_array_combine_result {
  int64_t  clipped;      /* stored components whose rint(.) lay outside dst's integer range */
  uint64_t sum_sq;       /* exact sum of the squares of the stored components */
} gc_array_combine_result;  /* 16 bytes */
int gc_array_combine(gc_context* const* srcs, gc_context* dst, const gc_array_combine_params* p,
                     const double* weights /* [K][T][2] = {re, im} */, gc_array_combine_result* res /* may be NULL */);
/* Test hook (host code only, no context): samples a workgroup of either kernel takes (a tile), ntaps standing for nlags too; 0 for an
 * nrecords or ntaps out of range. */
long long gc_debug_array_tile_outputs(int nrecords, int ntaps);

#ifdef __cplusplus
}
#endif
#endif /* GNSSCORR_H */
