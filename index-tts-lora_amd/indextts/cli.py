"""`indextts` command line (same flags and exit codes as the reference's indextts/cli.py:10-58)."""
import os
import sys


def main(argv=None):
    import argparse
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
    parser.add_argument("-d", "--device", type=str, default=None, help="device (cuda:N); CPU/MPS are not supported")
    args = parser.parse_args(argv)

    def fail(msg):
        print(f"[error] {msg}")
        parser.print_help()
        sys.exit(1)

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
    tts = IndexTTS(cfg_path=args.config, model_dir=args.model_dir, is_fp16=args.fp16, device=args.device)
    if args.stream:
        from indextts.utils.audio import write_pcm16
        rate, chunks = 24000, []
        for rate, pcm in tts.infer_stream(audio_prompt=args.voice, text=args.text.strip(), parallel_sentences=args.stream_parallel,
                                            **({} if args.stream_slots is None else {"slots": args.stream_slots}),
                                            **({"latent_cache": True} if args.stream_latent_cache else {})):
            chunks.append(pcm.cpu())
        if os.path.dirname(args.output_path) != "":
            os.makedirs(os.path.dirname(args.output_path), exist_ok=True)
        wav = torch.cat(chunks) if chunks else torch.zeros(0)
        write_pcm16(args.output_path, wav.to(torch.float32).numpy().astype("int16"), rate)
        print(f">> [output] saved to: {args.output_path}")
        return
    tts.infer(audio_prompt=args.voice, text=args.text.strip(), output_path=args.output_path)


if __name__ == "__main__":
    main()
