/*
 * vox_hip_transcribe -- main.c's file mode (main.c:107-118, 126-210, 383-410) on the
 * MI355X backend through the C host API (include/vox_hip_host.h):
 *
 *   vox_hip_transcribe -d consolidated.safetensors -i audio.wav [-I secs] [--delay ms]
 *                      [--alt cutoff] [--continuous] [--mx4] [--kv8] [--enc-kv16 | --enc-kv8]
 *                      [--q8-gemmf] [--kv-grow slots]
 *
 * The audio is fed in pieces of min(interval, 1 s) of samples, as main.c's feed_and_drain
 * does; every generated token id is printed to stdout (the tokenizer is out of scope) --
 * with --alt (main.c:149-154, 3 candidates) as id|alt|alt for the accepted alternatives.
 * --continuous turns on live mode (vox_stream_set_continuous, which main.c sets for --stdin
 * and the microphone, main.c:208-209) on the file's samples.  --mx4 (no reference
 * counterpart) rounds the decoder's matrices to MXFP4 values at load and streams them as such
 * in the single-stream decode step (vox_hip_set_wmx4(2), voxtral_hip.h; a checkpoint that is
 * already MXFP4-valued needs only VOX_HIP_WMX4=1); one stderr line reports what was built.
 * --kv8 (no reference counterpart) keeps the decoder KV rings in FP8 E4M3 (vh_set_kv_dtype(ctx, 2):
 * a quarter of the f32 rings' bytes, no scale, effect on transcripts not evaluated).
 * --enc-kv16 (no reference counterpart) keeps the encoder KV rings in IEEE half
 * (vh_set_enc_kv_fp16(ctx, 1): half of the f32 rings' bytes, effect on transcripts not evaluated).
 * --enc-kv8 (no reference counterpart) keeps them in FP8 E4M3 instead (vh_set_enc_kv_dtype(ctx, 2): a
 * quarter of the f32 rings' bytes, no scale, effect on transcripts not evaluated); giving both
 * --enc-kv16 and --enc-kv8 is an error.
 * --kv-grow N (no reference counterpart) starts the decoder KV rings at N slots (clamped to 64..
 * window + 64) and lets them double as the stream's position needs them (vh_set_kv_grow(ctx, N):
 * lossless, the same tokens; one slot is 80 ms of audio).
 * --q8-gemmf (no reference counterpart) puts a Q8 checkpoint's encoder passes and decoder
 * prefill on the stream-K MFMA GEMM over its int8 fragment copies (vox_hip_set_gemmf_q8(1),
 * voxtral_hip.h: the f32 summation order of those passes changes, nothing else).  The
 * reference's stderr lines ("Audio:", "Encoder:", "Decoder:") are kept so its
 * benchmark.py regexes parse this program's output too.
 */
#include "../../include/vox_hip_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define DEFAULT_FEED_CHUNK 16000  /* main.c: 1 s of samples */

static void drain(vh_stream_t *s, int *text_tokens, int alt) {
    int rec[256 * VH_MAX_ALT], n;
    while ((n = vh_stream_get_alt(s, rec, 256)) > 0)
        for (int i = 0; i < n; i++) {
            const int *r = rec + i * VH_MAX_ALT;
            printf("%d", r[0]);
            for (int a = 1; alt && a < VH_MAX_ALT && r[a] >= 0; a++) printf("|%d", r[a]);
            printf(" ");
            if (vh_token_class(r[0]) == VH_TOK_TEXT) (*text_tokens)++;
        }
    fflush(stdout);
}

int main(int argc, char **argv) {
    const char *model = NULL, *wav = NULL;
    float interval = -1.0f, alt_cutoff = -1.0f;
    int delay_ms = -1, continuous = 0, mx4 = 0, kv8 = 0, enc_kv16 = 0, enc_kv8 = 0, q8_gemmf = 0, kv_grow = 0;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-d") && i + 1 < argc) model = argv[++i];
        else if (!strcmp(argv[i], "-i") && i + 1 < argc) wav = argv[++i];
        else if (!strcmp(argv[i], "-I") && i + 1 < argc) interval = (float)atof(argv[++i]);
        else if (!strcmp(argv[i], "--delay") && i + 1 < argc) delay_ms = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--alt") && i + 1 < argc) alt_cutoff = (float)atof(argv[++i]);
        else if (!strcmp(argv[i], "--continuous")) continuous = 1;
        else if (!strcmp(argv[i], "--mx4")) mx4 = 1;
        else if (!strcmp(argv[i], "--kv8")) kv8 = 1;
        else if (!strcmp(argv[i], "--enc-kv16")) enc_kv16 = 1;
        else if (!strcmp(argv[i], "--enc-kv8")) enc_kv8 = 1;
        else if (!strcmp(argv[i], "--q8-gemmf")) q8_gemmf = 1;
        else if (!strcmp(argv[i], "--kv-grow") && i + 1 < argc) kv_grow = atoi(argv[++i]);
        else {
            model = NULL;
            break;
        }
    }
    if (enc_kv16 && enc_kv8) {
        fprintf(stderr, "%s: --enc-kv16 and --enc-kv8 exclude each other\n", argv[0]);
        model = NULL;
    }
    if (!model || !wav || kv_grow < 0 || (alt_cutoff != -1.0f && (alt_cutoff < 0 || alt_cutoff > 1))) {
        fprintf(stderr, "usage: %s -d consolidated.safetensors -i audio.wav [-I secs] [--delay ms] "
                        "[--alt 0..1] [--continuous] [--mx4] [--kv8] [--enc-kv16 | --enc-kv8] [--q8-gemmf] [--kv-grow slots]\n",
                argv[0]);
        return 2;
    }
    if (mx4 && vox_hip_set_wmx4(2)) return 1;
    if (q8_gemmf && vox_hip_set_gemmf_q8(1)) return 1;
    vh_ctx_t *ctx = vh_load(model);
    if (!ctx) return 1;
    if (vox_hip_wmx4()) {
        vox_hip_wmx4_stats_t ms;
        if (vox_hip_model_wmx4_stats(vh_model(ctx), &ms)) return 1;
        fprintf(stderr, "wmx4: mode %d, %d tensors streamed as MXFP4 (%d refused), %.1f MB for %.1f MB of bf16, "
                        "%.2f bits/weight; scan %.0f ms, round %.0f ms, pack %.0f ms\n",
                vox_hip_wmx4(), ms.wmx4_tensors, ms.refused_tensors, ms.plane_bytes / 1e6, ms.bf16_bytes / 1e6,
                ms.bits_per_weight, ms.scan_ms, ms.round_ms, ms.pack_ms);
    }
    if (kv8 && vh_set_kv_dtype(ctx, 2)) return 1;
    if (enc_kv16 && vh_set_enc_kv_fp16(ctx, 1)) return 1;
    if (enc_kv8 && vh_set_enc_kv_dtype(ctx, 2)) return 1;
    if (kv_grow && vh_set_kv_grow(ctx, kv_grow)) return 1;
    if (delay_ms > 0 && vh_set_delay(ctx, delay_ms)) return 1;
    vh_stream_t *s = vh_stream_init(ctx);
    if (!s) return 1;
    if (alt_cutoff >= 0 && vh_stream_set_alt(s, 3, alt_cutoff)) return 1;  /* main.c:197-198 */
    vh_stream_set_continuous(s, continuous);
    int feed_chunk = DEFAULT_FEED_CHUNK;
    if (interval > 0) {
        vh_set_processing_interval(s, interval);
        feed_chunk = (int)(interval * 16000);
        if (feed_chunk < 160) feed_chunk = 160;
        if (feed_chunk > DEFAULT_FEED_CHUNK) feed_chunk = DEFAULT_FEED_CHUNK;
    }
    int n = 0;
    float *samples = vh_load_wav(wav, &n);
    if (!samples) return 1;
    fprintf(stderr, "Audio: %d samples (%.1f seconds)\n", n, (float)n / 16000.0f);
    int text_tokens = 0, rc = 0;
    for (int off = 0; off < n && !rc; off += feed_chunk) {
        const int chunk = n - off < feed_chunk ? n - off : feed_chunk;
        rc = vh_stream_feed(s, samples + off, chunk);
        drain(s, &text_tokens, alt_cutoff >= 0);
    }
    free(samples);
    if (!rc) rc = vh_stream_finish(s);
    drain(s, &text_tokens, alt_cutoff >= 0);
    printf("\n");
    vh_stats_t st;
    vh_stream_stats(s, &st);
    /* the lines vox_stream_free prints (voxtral.c:1358-1370) */
    fprintf(stderr, "Encoder: %d mel -> %d tokens (%.0f ms)\n", st.mel_frames, st.adapter_tokens, st.encoder_ms);
    if (continuous) fprintf(stderr, "Restarts: %d (%d full)\n", st.restarts, st.full_resets);
    if (st.generated > 0) {
        const double gen_ms = st.decoder_ms - st.prefill_ms;
        fprintf(stderr, "Decoder: %d text tokens (%d steps) in %.0f ms (prefill %.0f ms + %.1f ms/step)\n",
                text_tokens, st.generated, st.decoder_ms, st.prefill_ms,
                st.generated > 1 ? gen_ms / (st.generated - 1) : 0.0);
    }
    vh_stream_free(s);
    vh_free(ctx);
    return rc ? 1 : 0;
}
