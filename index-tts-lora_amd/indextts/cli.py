"""`indextts` command line (same flags and exit codes as the reference's indextts/cli.py:10-58)."""
import os
import sys


def extract_voice_main(argv):
    """`indextts --extract-voice CKPT --voice-out FILE [--voice-max-rank R]`: recover the LoRA voice a merged fine-tuned checkpoint
    holds against this model's base weights (IndexTTS.voice_from_checkpoint) and save it (IndexTTS.save_voice).  A command of its
    own with its own arguments: the synthesis command line below is what it was."""
    import argparse
    parser = argparse.ArgumentParser(prog="indextts --extract-voice", description="IndexTTS: a voice file from a merged fine-tuned checkpoint")
    parser.add_argument("--extract-voice", type=str, required=True, metavar="CKPT", help="merged fine-tuned checkpoint (gpt_finetuned.pth)")
    parser.add_argument("--voice-out", type=str, required=True, metavar="FILE", help="the voice file to write (IndexTTS.load_voice reads it)")
    parser.add_argument("--voice-max-rank", type=int, default=16, metavar="R", help="the largest LoRA rank looked for (1..64)")
    parser.add_argument("-c", "--config", type=str, default="checkpoints/config.yaml", help="config file")
    parser.add_argument("--model_dir", type=str, default="checkpoints", help="model directory (holds the base gpt.pth)")
    parser.add_argument("--fp16", action="store_true", default=True, help="half-precision GPT weights when available")
    parser.add_argument("-f", "--force", action="store_true", default=False, help="overwrite the voice file")
    parser.add_argument("-d", "--device", type=str, default=None, help="device (cuda:N); CPU/MPS are not supported")
    args = parser.parse_args(argv)

    def fail(msg):
        print(f"[error] {msg}")
        parser.print_help()
        sys.exit(1)

    if not os.path.exists(args.extract_voice):
        fail(f"checkpoint {args.extract_voice} does not exist")
    if not 1 <= args.voice_max_rank <= 64:
        fail("--voice-max-rank must lie in [1, 64]")
    if not os.path.exists(args.config):
        fail(f"config {args.config} does not exist")
    if os.path.exists(args.voice_out) and not args.force:
        fail(f"voice file {args.voice_out} exists; use --force to overwrite")
    import torch
    if args.device is None:
        if not torch.cuda.is_available():
            print("[error] no GPU visible: this build needs an AMD GPU (no CPU path)")
            sys.exit(1)
        args.device = "cuda:0"
    from indextts.infer import IndexTTS
    tts = IndexTTS(cfg_path=args.config, model_dir=args.model_dir, is_fp16=args.fp16, device=args.device)
    try:
        adapters, scaling, report = tts.voice_from_checkpoint(args.extract_voice, max_rank=args.voice_max_rank, return_report=True)
    except ValueError as e:
        print(f"[error] {e}")
        sys.exit(1)
    for key, rep in report.items():
        print(f">> {key}: rank {rep['r']}, sigma_r {rep['sigma_r']:.4g}, sigma_r+1 {rep['sigma_next']:.4g}, ratio {rep['ratio']:.4g}")
    tts.save_voice(args.voice_out, adapters, scaling)
    print(f">> [voice] {len(adapters)} targets saved to: {args.voice_out}")


def extract_codes_main(argv):
    """`indextts --extract-codes LIST --out DIR`: the mel codes and mels of every clip of an audio list (`path<TAB>transcript` per
    line), the first step of the fine-tuning workflow (IndexTTS.extract_codes).  A command of its own with its own arguments."""
    import argparse
    parser = argparse.ArgumentParser(prog="indextts --extract-codes", description="IndexTTS: mel codes and mels of an audio list")
    parser.add_argument("--extract-codes", type=str, required=True, metavar="LIST", help="audio list: path<TAB>transcript per line")
    parser.add_argument("--out", type=str, required=True, metavar="DIR", help="directory for codes/, mels/ and metadata.jsonl")
    parser.add_argument("--dvae", type=str, default=None, metavar="CKPT", help="DVAE checkpoint (default: the config's dvae_checkpoint)")
    parser.add_argument("--batch-clips", type=int, default=16, metavar="N", help="clips per ragged batch")
    parser.add_argument("-c", "--config", type=str, default="checkpoints/config.yaml", help="config file")
    parser.add_argument("--model_dir", type=str, default="checkpoints", help="model directory")
    parser.add_argument("--fp16", action="store_true", default=True, help="half-precision GPT weights when available")
    parser.add_argument("--prompt-frontend", choices=("torch", "hip"), default="hip", help="where the log-mel is computed")
    parser.add_argument("-d", "--device", type=str, default=None, help="device (cuda:N); CPU/MPS are not supported")
    args = parser.parse_args(argv)

    def fail(msg):
        print(f"[error] {msg}")
        parser.print_help()
        sys.exit(1)

    if not os.path.exists(args.extract_codes):
        fail(f"audio list {args.extract_codes} does not exist")
    if args.batch_clips < 1:
        fail("--batch-clips must be at least 1")
    if not os.path.exists(args.config):
        fail(f"config {args.config} does not exist")
    import torch
    if args.device is None:
        if not torch.cuda.is_available():
            print("[error] no GPU visible: this build needs an AMD GPU (no CPU path)")
            sys.exit(1)
        args.device = "cuda:0"
    from indextts.infer import IndexTTS
    tts = IndexTTS(cfg_path=args.config, model_dir=args.model_dir, is_fp16=args.fp16, device=args.device, prompt_frontend=args.prompt_frontend)
    try:
        tts.load_tokenizer(args.dvae)
        records = tts.extract_codes(args.extract_codes, args.out, batch_clips=args.batch_clips)
    except (ValueError, OSError, RuntimeError) as e:
        print(f"[error] {e}")
        sys.exit(1)
    print(f">> [codes] {len(records)} clips, {sum(r['duration'] for r in records):.1f} s of audio -> {args.out}")


def score_rows(tts, cond_mel, items, voice_ids=(None,), voice_names=(None,), batch_clips=16):
    """The records of `indextts --score`: for every clip of items [(path, transcript)] and every voice one dict -- audio, text, voice
    and the fields of IndexTTS.score_codes with the arrays as lists.  The clips' codes are taken once per chunk
    (IndexTTS.audio_codes) and scored under each voice in turn."""
    step = max(1, int(batch_clips))
    for at in range(0, len(items), step):
        chunk = items[at: at + step]
        codes, _ = tts.audio_codes([p for p, _ in chunk])
        rows = [tts.text_token_row(t) for _, t in chunk]
        for vid, vname in zip(voice_ids, voice_names):
            recs = tts.score_codes(cond_mel, rows, codes, adapter_ids=None if vid is None else [vid] * len(chunk))
            for (path, text), r in zip(chunk, recs):
                yield dict(audio=path, text=text, voice=vname, **{k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in r.items()})


def read_audio_list(path):
    """[(audio path, transcript)] of a `path<TAB>transcript` list; a relative audio path is relative to the list."""
    base = os.path.dirname(os.path.abspath(path))
    items = []
    with open(path, "r", encoding="utf-8") as f:
        for n, line in enumerate(f):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            audio, tab, text = line.partition("\t")
            if not tab or not audio.strip():
                raise ValueError(f"{path}:{n + 1}: expected `path<TAB>transcript`")
            audio = audio.strip()
            items.append((audio if os.path.isabs(audio) else os.path.join(base, audio), text.strip()))
    return items


def score_main(argv):
    """`indextts --score LIST -v PROMPT --out FILE.jsonl [--voices FILE ...]`: how likely is every clip of an audio list
    (`path<TAB>transcript` per line, the format of --extract-codes) under the model -- and, with --voices, under each voice file
    (IndexTTS.load_voice) -- in the voice of the prompt: one JSON line per clip and voice (score_rows).  -v is required: the
    decoder scores codes in the voice of a reference recording, as it synthesises them."""
    import argparse
    import json
    parser = argparse.ArgumentParser(prog="indextts --score", description="IndexTTS: likelihood of recordings' mel codes")
    parser.add_argument("--score", type=str, required=True, metavar="LIST", help="audio list: path<TAB>transcript per line")
    parser.add_argument("--out", type=str, required=True, metavar="FILE.jsonl", help="one JSON record per clip and voice")
    parser.add_argument("-v", "--voice", type=str, required=True, help="reference (prompt) audio file, wav")
    parser.add_argument("--voices", type=str, nargs="*", default=[], metavar="FILE", help="voice files (--extract-voice); none: the base model")
    parser.add_argument("--dvae", type=str, default=None, metavar="CKPT", help="DVAE checkpoint (default: the config's dvae_checkpoint)")
    parser.add_argument("--batch-clips", type=int, default=16, metavar="N", help="clips per ragged batch")
    parser.add_argument("-c", "--config", type=str, default="checkpoints/config.yaml", help="config file")
    parser.add_argument("--model_dir", type=str, default="checkpoints", help="model directory")
    parser.add_argument("--fp32", action="store_true", default=False, help="fp32 GPT weights (default: half precision when available)")
    parser.add_argument("-d", "--device", type=str, default=None, help="device (cuda:N); CPU/MPS are not supported")
    args = parser.parse_args(argv)
    for path, what in ((args.score, "audio list"), (args.voice, "prompt"), (args.config, "config")) + tuple((v, "voice file") for v in args.voices):
        if not os.path.exists(path):
            print(f"[error] {what} {path} does not exist")
            sys.exit(1)
    if args.batch_clips < 1:
        print("[error] --batch-clips must be at least 1")
        sys.exit(1)
    try:
        items = read_audio_list(args.score)
    except ValueError as e:
        print(f"[error] {e}")
        sys.exit(1)
    import torch
    if args.device is None:
        if not torch.cuda.is_available():
            print("[error] no GPU visible: this build needs an AMD GPU (no CPU path)")
            sys.exit(1)
        args.device = "cuda:0"
    from indextts.infer import IndexTTS
    tts = IndexTTS(cfg_path=args.config, model_dir=args.model_dir, is_fp16=not args.fp32, device=args.device)
    try:
        tts.load_tokenizer(args.dvae)
        cond_mel = tts.prompt_mels([args.voice])[0]
        ids, names = [None], [None]
        if args.voices:
            loaded = [tts.load_voice(v) for v in args.voices]
            rank = max(int(A.shape[0]) for ad, _ in loaded for A, _ in ad.values())
            # the pool's limit is slots x (rank padded to 16) <= 512; a batch scores under ONE voice, so few slots do
            tts.attach_voice_pool(slots=max(1, min(len(loaded), 512 // ((rank + 15) // 16 * 16))), rank=rank)
            ids, names = [tts.add_voice(ad, sc) for ad, sc in loaded], list(args.voices)
        n = 0
        with open(args.out, "w", encoding="utf-8") as f:
            for rec in score_rows(tts, cond_mel, items, ids, names, args.batch_clips):
                f.write(json.dumps(rec, ensure_ascii=False) + "\n")
                n += 1
    except (ValueError, OSError, RuntimeError) as e:
        print(f"[error] {e}")
        sys.exit(1)
    print(f">> [score] {n} records -> {args.out}")


def fit_voice_parser():
    """The argument parser of `indextts --fit-voice` (a function of its own: the parsing is tested without a device)."""
    import argparse
    parser = argparse.ArgumentParser(prog="indextts --fit-voice", description="IndexTTS: fit a LoRA voice to a directory of codes")
    parser.add_argument("--fit-voice", type=str, required=True, metavar="DIR", help="what --extract-codes wrote: metadata.jsonl, codes/")
    parser.add_argument("-v", "--voice", type=str, required=True, help="reference (prompt) audio file, wav")
    parser.add_argument("--out", type=str, required=True, metavar="VOICE.pt", help="the voice file to write (IndexTTS.load_voice reads it)")
    parser.add_argument("--rank", type=int, default=4, metavar="R", help="LoRA rank (1..64)")
    parser.add_argument("--alpha", type=float, default=8.0, help="LoRA alpha (the scaling is alpha / rank)")
    parser.add_argument("--steps", type=int, default=100, metavar="N", help="optimizer steps")
    parser.add_argument("--lr", type=float, default=5.0e-6, help="learning rate of the A factors (B: twice it, LoRA+)")
    parser.add_argument("--batch-rows", type=int, default=4096, metavar="ROWS", help="rows (utterances x the longest) of one padded batch")
    parser.add_argument("--text-weight", type=float, default=0.1, help="weight of the text loss (the mel loss: one minus it)")
    parser.add_argument("--dropout", type=float, default=0.2, help="LoRA dropout")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--save-merged", type=str, default=None, metavar="PATH", help="also write the merged checkpoint (gpt_finetuned.pth format)")
    parser.add_argument("--fit-attention", type=str, default="torch", choices=("torch", "hip"),
                        help="the fit's causal attention: the torch loop, or the ragged HIP kernels (forward and backward)")
    parser.add_argument("-c", "--config", type=str, default="checkpoints/config.yaml", help="config file")
    parser.add_argument("--model_dir", type=str, default="checkpoints", help="model directory")
    parser.add_argument("--fp32", action="store_true", default=False, help="fp32 GPT weights (default: half precision when available)")
    parser.add_argument("-f", "--force", action="store_true", default=False, help="overwrite the voice file")
    parser.add_argument("-d", "--device", type=str, default=None, help="device (cuda:N); CPU/MPS are not supported")
    return parser


def fit_voice_main(argv):
    """`indextts --fit-voice DIR -v PROMPT --out VOICE.pt [--rank --alpha --steps --lr --batch-rows --text-weight --dropout --seed
    --save-merged PATH --fit-attention torch|hip]`: train a LoRA voice on the codes of a directory (IndexTTS.fit_voice_from_dir) and save it."""
    parser = fit_voice_parser()
    args = parser.parse_args(argv)

    def fail(msg):
        print(f"[error] {msg}")
        parser.print_help()
        sys.exit(1)

    if not os.path.exists(os.path.join(args.fit_voice, "metadata.jsonl")):
        fail(f"{args.fit_voice} holds no metadata.jsonl (run --extract-codes first)")
    for path, what in ((args.voice, "prompt"), (args.config, "config")):
        if not os.path.exists(path):
            fail(f"{what} {path} does not exist")
    if not 1 <= args.rank <= 64:
        fail("--rank must lie in [1, 64]")
    if args.steps < 1 or args.batch_rows < 1:
        fail("--steps and --batch-rows must be at least 1")
    if os.path.exists(args.out) and not args.force:
        fail(f"voice file {args.out} exists; use --force to overwrite")
    import torch
    if args.device is None:
        if not torch.cuda.is_available():
            print("[error] no GPU visible: this build needs an AMD GPU (no CPU path)")
            sys.exit(1)
        args.device = "cuda:0"
    from indextts.infer import IndexTTS
    tts = IndexTTS(cfg_path=args.config, model_dir=args.model_dir, is_fp16=not args.fp32, device=args.device)
    try:
        cond_mel = tts.prompt_mels([args.voice])[0]
        adapters, scaling, report = tts.fit_voice_from_dir(
            args.fit_voice, cond_mel, rank=args.rank, alpha=args.alpha, steps=args.steps, lr=args.lr, batch_rows=args.batch_rows,
            text_weight=args.text_weight, dropout=args.dropout, seed=args.seed, return_report=True, attention=args.fit_attention)
    except (ValueError, OSError, RuntimeError) as e:
        print(f"[error] {e}")
        sys.exit(1)
    first, last = report["steps"][0], report["steps"][-1]
    print(f">> [fit] {len(report['steps'])} steps: loss_mel {first['loss_mel']:.4f} -> {last['loss_mel']:.4f}, "
          f"loss_text {first['loss_text']:.4f} -> {last['loss_text']:.4f}")
    tts.save_voice(args.out, adapters, scaling)
    print(f">> [voice] {len(adapters)} targets saved to: {args.out}")
    if args.save_merged:
        tts.save_merged(args.save_merged, adapters, scaling)
        print(f">> [merged] saved to: {args.save_merged}")


def main(argv=None):
    import argparse
    argv = sys.argv[1:] if argv is None else list(argv)
    if any(a == "--fit-voice" or a.startswith("--fit-voice=") for a in argv):
        return fit_voice_main(argv)
    if any(a == "--extract-voice" or a.startswith("--extract-voice=") for a in argv):
        return extract_voice_main(argv)
    if any(a == "--extract-codes" or a.startswith("--extract-codes=") for a in argv):
        return extract_codes_main(argv)
    if any(a == "--score" or a.startswith("--score=") for a in argv):
        return score_main(argv)
    parser = argparse.ArgumentParser(description="IndexTTS command line (MI355X build)")
    parser.add_argument("text", type=str, help="text to synthesise")
    parser.add_argument("-v", "--voice", type=str, required=True, help="reference (prompt) audio file, wav")
    parser.add_argument("-o", "--output_path", type=str, default="gen.wav", help="output wav path")
    parser.add_argument("-c", "--config", type=str, default="checkpoints/config.yaml", help="config file")
    parser.add_argument("--model_dir", type=str, default="checkpoints", help="model directory")
    parser.add_argument("--fp16", action="store_true", default=True, help="half-precision GPT weights when available")
    parser.add_argument("-f", "--force", action="store_true", default=False, help="overwrite the output file")
    parser.add_argument("--stream", action="store_true", default=False,
                        help="synthesise chunk by chunk while the token loop runs (IndexTTS.infer_stream) and write the chunks to the same "
                             "path in the same format; the stream samples with num_beams = 1 (the default path keeps 3 beams), so "
                             "the samples differ from a run without this flag")
    parser.add_argument("--stream-parallel", type=int, default=1, metavar="P",
                        help="with --stream: up to P sentences of the text share one token loop (IndexTTS.infer_stream("
                             "parallel_sentences=P)); the chunks are still written in text order.  1 streams sentence by sentence")
    parser.add_argument("--stream-slots", type=int, default=None, metavar="S",
                        help="with --stream: ALL sentences of the text go through one refilled loop of S decode slots "
                             "(IndexTTS.infer_stream(slots=S)): a sentence that ends hands its slot to the next one.  The chunks are "
                             "still written in text order; --stream-parallel does not apply then")
    parser.add_argument("--stream-latent-cache", action="store_true", default=False,
                        help="with --stream: keep the latent pass's keys and values between chunks (IndexTTS.infer_stream("
                             "latent_cache=True)): a chunk boundary then costs its new rows only")
    parser.add_argument("--prompt-frontend", choices=("torch", "hip"), default="torch",
                        help="where the prompt's wav becomes its log-mel: torch (host ops, the default) or hip (the device "
                             "front-end, IndexTTS(prompt_frontend='hip'))")
    parser.add_argument("--sample-rate", type=int, default=None, metavar="HZ",
                        help="sample rate of the output file (8000, 16000, 44100, 48000, ...; resampled on the device, "
                             "IndexTTS.output_format).  Default: 24000, the vocoder's")
    parser.add_argument("--encoding", choices=("pcm16", "f32", "mulaw", "alaw"), default=None,
                        help="sample encoding of the output file: 16-bit PCM (the default), IEEE float, or G.711 mu-law / A-law")
    parser.add_argument("--trim-db", type=float, default=None, metavar="DB",
                        help="cut leading and trailing silence: a 10 ms frame below this level (dBFS, e.g. -45) is silent "
                             "(on the device, IndexTTS.post_process).  Default: nothing is cut")
    parser.add_argument("--max-pause-ms", type=float, default=None, metavar="MS",
                        help="shorten an inner pause longer than this to it (needs --trim-db)")
    parser.add_argument("--target-rms-db", type=float, default=None, metavar="DB",
                        help="bring the RMS of the speech to this level (dBFS, e.g. -20); the peak stays under --peak-db")
    parser.add_argument("--peak-db", type=float, default=None, metavar="DB",
                        help="peak ceiling (dBFS; -1 under --target-rms-db); alone: peak normalisation")
    parser.add_argument("--speed", type=float, default=None, metavar="X",
                        help="speaking rate, 0.5 to 2.0: 0.8 is a fifth slower, 1.25 a quarter faster, at the same pitch (WSOLA on "
                             "the device, IndexTTS.infer(speed=...)).  Default: the voice as it is")
    parser.add_argument("--pitch", type=float, default=None, metavar="SEMITONES",
                        help="pitch, -12 to 12 semitones: 2 is a whole tone up, at the duration --speed sets (WSOLA and a resampler on "
                             "the device, IndexTTS.infer(pitch=...)); the formants move with it.  Default: the voice as it is")
    parser.add_argument("-d", "--device", type=str, default=None, help="device (cuda:N); CPU/MPS are not supported")
    args = parser.parse_args(argv)

    def fail(msg):
        print(f"[error] {msg}")
        parser.print_help()
        sys.exit(1)

    output = None
    if args.sample_rate is not None or args.encoding is not None:
        from indextts.utils.pcm_out import OutputFormat
        try:
            output = OutputFormat(24000 if args.sample_rate is None else args.sample_rate, args.encoding or "pcm16")
        except ValueError as e:
            fail(str(e))
    post = None
    if any(v is not None for v in (args.trim_db, args.max_pause_ms, args.target_rms_db, args.peak_db)):
        if args.stream:
            fail("--trim-db, --max-pause-ms, --target-rms-db and --peak-db do not apply to --stream: the level of a whole "
                 "utterance is not known at its first chunk")
        from indextts.utils.post_wave import PostProcess
        try:
            post = PostProcess(trim_db=args.trim_db, max_pause_ms=args.max_pause_ms, target_rms_db=args.target_rms_db, peak_db=args.peak_db)
        except ValueError as e:
            fail(str(e))
    if args.speed is not None:
        if args.stream:
            fail("--speed does not apply to --stream: the chain of lags is not carried across chunk boundaries")
        from indextts.utils.tempo import fixed_speed
        try:
            fixed_speed(args.speed)
        except ValueError as e:
            fail(f"--speed: {e}")
    if args.pitch is not None:
        if args.stream:
            fail("--pitch does not apply to --stream: the chain of lags is not carried across chunk boundaries")
        from indextts.utils.tempo import pitch_plan
        try:
            pitch_plan(args.pitch, args.speed)
        except ValueError as e:
            fail(f"--pitch: {e}")
    if len(args.text.strip()) == 0:
        fail("text is empty")
    if args.stream_parallel < 1:
        fail("--stream-parallel must be at least 1")
    if args.stream_slots is not None and args.stream_slots < 1:
        fail("--stream-slots must be at least 1")
    if not os.path.exists(args.voice):
        fail(f"reference audio {args.voice} does not exist")
    if not os.path.exists(args.config):
        fail(f"config {args.config} does not exist")
    if os.path.exists(args.output_path):
        if not args.force:
            fail(f"output file {args.output_path} exists; use --force to overwrite")
        os.remove(args.output_path)
    try:
        import torch
    except ImportError:
        print("[error] PyTorch is not installed")
        sys.exit(1)
    if args.device is None:
        if not torch.cuda.is_available():
            print("[error] no GPU visible: this build needs an AMD GPU (no CPU path)")
            sys.exit(1)
        args.device = "cuda:0"
    from indextts.infer import IndexTTS
    tts = IndexTTS(cfg_path=args.config, model_dir=args.model_dir, is_fp16=args.fp16, device=args.device,
                   prompt_frontend=args.prompt_frontend)
    if args.stream:
        from indextts.utils.audio import write_pcm16
        rate, chunks = 24000, []
        for rate, pcm in tts.infer_stream(audio_prompt=args.voice, text=args.text.strip(), parallel_sentences=args.stream_parallel,
                                            **({} if args.stream_slots is None else {"slots": args.stream_slots}),
                                            **({"latent_cache": True} if args.stream_latent_cache else {}),
                                            **({} if output is None else {"output": output})):
            chunks.append(pcm.cpu())
        if os.path.dirname(args.output_path) != "":
            os.makedirs(os.path.dirname(args.output_path), exist_ok=True)
        if output is not None:
            from indextts.utils.audio import write_wav
            wav = torch.cat(chunks) if chunks else torch.zeros(0, dtype=output.dtype)
            write_wav(args.output_path, wav.numpy(), output.sample_rate, output.encoding)
            print(f">> [output] saved to: {args.output_path}")
            return
        wav = torch.cat(chunks) if chunks else torch.zeros(0)
        write_pcm16(args.output_path, wav.to(torch.float32).numpy().astype("int16"), rate)
        print(f">> [output] saved to: {args.output_path}")
        return
    tts.infer(audio_prompt=args.voice, text=args.text.strip(), output_path=args.output_path, **({} if output is None else {"output": output}),
              **({} if post is None else {"post": post}), **({} if args.speed is None else {"speed": args.speed}),
              **({} if args.pitch is None else {"pitch": args.pitch}))


if __name__ == "__main__":
    main()
