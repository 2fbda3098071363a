"""HTTP front of the MI355X build: the reference's REST surface (api.py:35-300) over this package's IndexTTS.

    python index-tts-lora_amd/api.py --model_dir checkpoints --config checkpoints/config.yaml [--port 7859]

Same routes, request fields, defaults and status codes as the reference server, so a client written against it keeps
working:
    GET  /models          {"models": [{name, filename, type}], "current_model": ...}          (api.py:97-116)
    POST /model/reload    {"model_filename": ...} -> hot-swaps tts.gpt (404 when the file is missing)  (api.py:118-175)
    POST /tts/stream      /tts's request (not in the reference) -> chunked audio/L16; rate=24000 while the token loop runs, header X-Seed
                          (with the form fields sample_rate / encoding: audio/L16 | audio/PCMU | audio/PCMA | audio/L32F; rate=R,
                          resampled and encoded on the device; /tts takes the same fields and tags its WAV accordingly)
                          (--stream-slots S / create_app(stream_slots=S): all such requests share one refilled loop of S slots)
    POST /tts             text + prompt_audio (upload) | prompt_audio_path, infer_mode fast|normal, speaker_id, seed and the
                          generation knobs -> audio/wav, header X-Seed; 400 without a prompt, 404 for a missing prompt path,
                          503 before the engine is up, 500 with the error text otherwise                (api.py:177-300)
                          (with the fields trim_db / max_pause_ms / target_rms_db / peak_db: silence trimmed, pauses capped and the
                          level set on the device, IndexTTS.post_process; 400 for an out-of-range value, and on /tts/stream)
                          (with the field speed, 0.5 .. 2.0: the speaking rate at the same pitch, on the device before the
                          finishing, IndexTTS.infer(speed=...); 400 for an out-of-range value, and on /tts/stream)
                          (with the field pitch, -12 .. 12 semitones: the voice higher or lower at the duration speed sets, on the
                          device where speed is applied, IndexTTS.infer(pitch=...); an empty field is none; 400 for a value out
                          of range or one that takes speed / 2^(pitch / 12) outside 0.5 .. 2.0, and on /tts/stream)
/tts accepts the reference's multipart form (parsed with the standard library: python-multipart is optional), a urlencoded
form, or a JSON body with the same field names (the reference's TTSRequest model, api.py:35-50).  One engine instance per
process, requests are serialised by a lock (the reference's endpoints are effectively serial as well: one global
IndexTTS with per-instance caches)."""
from __future__ import annotations

import argparse
import json
import os
import queue
import random
import tempfile
import threading
import time
import urllib.parse
from email.parser import BytesParser
from typing import Optional

from fastapi import FastAPI, HTTPException, Request
from fastapi.concurrency import run_in_threadpool
from fastapi.responses import Response, StreamingResponse
from pydantic import BaseModel


class TTSRequest(BaseModel):
    """Field names and defaults of the reference's /tts form (api.py:178-195; the JSON model api.py:35-50 has the same names)."""
    text: str
    prompt_audio_path: Optional[str] = None
    infer_mode: str = "fast"   # 'normal' | 'fast'
    speaker_id: Optional[str] = None
    seed: Optional[int] = None
    max_text_tokens_per_sentence: int = 120
    sentences_bucket_max_size: int = 4
    do_sample: bool = True
    top_p: float = 0.8
    top_k: int = 30
    temperature: float = 0.3
    repetition_penalty: float = 10.0
    length_penalty: float = 0.0
    max_mel_tokens: int = 600
    sample_rate: Optional[int] = None      # None: 24000, the vocoder's rate
    encoding: Optional[str] = None         # None: pcm16; f32 | mulaw | alaw (IndexTTS.output_format)
    trim_db: Optional[float] = None        # /tts only (IndexTTS.post_process): frames below this level (dBFS) are silence; the ends are trimmed
    max_pause_ms: Optional[float] = None   # /tts only: an inner pause longer than this is shortened to it (needs trim_db)
    target_rms_db: Optional[float] = None  # /tts only: the RMS of the speech is brought to this level (dBFS)
    peak_db: Optional[float] = None        # /tts only: the peak ceiling (dBFS; -1 under a target); alone: peak normalisation
    speed: Optional[float] = None          # /tts only: the speaking rate, 0.5 .. 2.0 (1.25 a quarter faster), at the same pitch
    pitch: Optional[float] = None          # /tts only: semitones, -12 .. 12 (the formants move with it), at the duration speed sets


def output_of(req):
    """The OutputFormat a request names with sample_rate / encoding (None when it names neither: the answer is what it has
    always been); a value the device back-end does not produce is a 400."""
    if req.sample_rate is None and req.encoding is None:
        return None
    from indextts.utils.pcm_out import OutputFormat
    try:
        return OutputFormat(24000 if req.sample_rate is None else req.sample_rate, req.encoding or "pcm16")
    except ValueError as e:
        raise HTTPException(status_code=400, detail=str(e))


def pitch_of(req, streaming=False):
    """The pitch a request names with pitch, in semitones (None when it names none: the answer is what it has always been); a
    value outside [-12, 12], or one that with the request's speed takes the time stretch outside [0.5, 2.0], is a 400, and so
    is the field on /tts/stream -- the chain of lags is not carried across chunks."""
    if req.pitch is None:
        return None
    if streaming:
        raise HTTPException(status_code=400, detail="pitch: /tts/stream does not change the pitch (use /tts)")
    from indextts.utils.tempo import pitch_plan
    try:
        pitch_plan(req.pitch, req.speed)
    except ValueError as e:
        raise HTTPException(status_code=400, detail=str(e))
    return float(req.pitch)


def speed_of(req, streaming=False):
    """The speaking rate a request names with speed (None when it names none: the answer is what it has always been); a value
    outside [0.5, 2.0] is a 400, and so is the field on /tts/stream -- the chain of lags is not carried across chunks."""
    if req.speed is None:
        return None
    if streaming:
        raise HTTPException(status_code=400, detail="speed: /tts/stream does not change the speaking rate (use /tts)")
    from indextts.utils.tempo import fixed_speed
    try:
        fixed_speed(req.speed)
    except ValueError as e:
        raise HTTPException(status_code=400, detail=str(e))
    return float(req.speed)


POST_FIELDS = ("trim_db", "max_pause_ms", "target_rms_db", "peak_db")


def post_of(req, streaming=False):
    """The PostProcess a request names with trim_db / max_pause_ms / target_rms_db / peak_db (None when it names none: the answer
    is what it has always been); an out-of-range value is a 400, and so is any of them on /tts/stream -- the level of a whole
    utterance is not known at its first chunk."""
    given = {k: getattr(req, k) for k in POST_FIELDS if getattr(req, k) is not None}
    if not given:
        return None
    if streaming:
        raise HTTPException(status_code=400, detail=f"{', '.join(given)}: /tts/stream does not finish waveforms (use /tts)")
    from indextts.utils.post_wave import PostProcess
    try:
        return PostProcess(**given)
    except ValueError as e:
        raise HTTPException(status_code=400, detail=str(e))


def chunk_bytes(pcm, fmt):
    return pcm.float().cpu().numpy().astype("<i2").tobytes() if fmt is None else fmt.to_bytes(pcm)


class ModelReloadRequest(BaseModel):
    model_filename: str


def _parse_multipart(body: bytes, content_type: str):
    """multipart/form-data with the standard library: {name: str | (filename, bytes)}."""
    msg = BytesParser().parsebytes(b"Content-Type: " + content_type.encode() + b"\r\nMIME-Version: 1.0\r\n\r\n" + body)
    out = {}
    for part in msg.get_payload() if msg.is_multipart() else []:
        name = part.get_param("name", header="content-disposition")
        if name is None:
            continue
        filename = part.get_param("filename", header="content-disposition")
        data = part.get_payload(decode=True) or b""
        out[name] = (filename, data) if filename is not None else data.decode("utf-8")
    return out


def _inside(path: str, roots) -> bool:
    """True when `path` (symlinks resolved) lies in one of the directories `roots`."""
    real = os.path.realpath(path)
    for r in roots:
        rr = os.path.realpath(r)
        if real == rr or real.startswith(rr.rstrip(os.sep) + os.sep):
            return True
    return False


def create_app(tts=None, model_dir="checkpoints", config_path="checkpoints/config.yaml", device=None, use_fp16=True,
               finetune_dir=os.path.join("finetune_models", "checkpoints"), output_dir=os.path.join("outputs", "api"),
               prompt_dir="prompts", stream_slots=None, stream_latent_cache=False, prompt_frontend="torch"):
    """`tts`: a ready IndexTTS (tests, embedding) or None to build one from model_dir / config_path on first use.
    stream_slots = S (off by default): /tts/stream requests are served by ONE worker that owns a refilled streaming loop of S
    decode slots (IndexTTS.serve_stream_queue): a request that arrives while the loop runs enters it, a request that finds no
    loop starts one.  None: every /tts/stream request runs its own generation under the engine lock, as before.
    stream_latent_cache (off by default): /tts/stream runs the incremental latent pass (latent_cache=True of
    IndexTTS.infer_stream / serve_stream_queue) on either route.
    Server-side paths a client may name are confined (the reference opens whatever it is given, api.py:125-134, :218-226):
    /model/reload only loads files inside model_dir / finetune_dir, /tts prompt_audio_path only reads files inside
    prompt_dir / model_dir; anything else answers 403."""
    from indextts.infer import IndexTTS, set_seed

    app = FastAPI(title="IndexTTS API (MI355X build)", version="1.0.0")
    state = {"tts": tts}
    lock = threading.Lock()
    latent_kw = {"latent_cache": True} if stream_latent_cache else {}
    model_roots = [model_dir, finetune_dir]
    prompt_roots = [prompt_dir, model_dir]

    def engine():
        if state["tts"] is None:
            if not os.path.exists(model_dir):
                raise HTTPException(status_code=503, detail=f"model directory {model_dir} does not exist")
            state["tts"] = IndexTTS(model_dir=model_dir, cfg_path=config_path, device=device, is_fp16=use_fp16,
                                    prompt_frontend=prompt_frontend)
        return state["tts"]

    app.state.engine = engine

    @app.get("/models")
    def list_models():
        models = []
        if os.path.exists(os.path.join(model_dir, "gpt.pth")):
            models.append({"name": "Default (gpt.pth)", "filename": "gpt.pth", "type": "base"})
        if os.path.exists(finetune_dir):
            for f in sorted(os.listdir(finetune_dir)):
                if f.endswith(".pth"):
                    models.append({"name": f"Finetuned - {f}", "filename": os.path.join(finetune_dir, f), "type": "finetune"})
        t = state["tts"]
        return {"models": models, "current_model": os.path.basename(t.gpt_path) if t is not None and t.gpt_path else "None"}

    @app.post("/model/reload")
    def reload_model(request: ModelReloadRequest):
        model_path = request.model_filename
        if not os.path.isabs(model_path):
            if os.path.exists(os.path.join(model_dir, model_path)):
                model_path = os.path.join(model_dir, model_path)
            elif not os.path.exists(model_path):
                raise HTTPException(status_code=404, detail=f"model file {model_path} does not exist")
        elif not os.path.exists(model_path):
            raise HTTPException(status_code=404, detail=f"model file {model_path} does not exist")
        if not _inside(model_path, model_roots):
            raise HTTPException(status_code=403, detail="model files are only loaded from the model / fine-tune directories")
        try:
            with lock:
                engine().reload_gpt(model_path)
            return {"status": "success", "message": f"switched to model: {os.path.basename(model_path)}"}
        except HTTPException:
            raise
        except Exception as e:  # noqa: BLE001
            raise HTTPException(status_code=500, detail=str(e))

    class SharedStreamLoop:
        """The worker of stream_slots: requests wait in `inbox`; one thread at a time holds the engine lock and runs a
        serve_stream_queue loop, whose more() empties the inbox at every boundary.  The loop ends when it has fallen idle; a
        request that arrives after that starts the next thread.  The lock is held for the loop only, never while anything waits
        for a client: the chunks go to each request's own queue."""

        def __init__(self):
            self.mutex, self.inbox, self.running, self.jobs, self.count = threading.Lock(), [], False, {}, 0
            self.outs = {}       # handle -> [its OutputFormat, its PcmOutStream once its first chunk has come]

        def submit(self, request, chunks, done, fmt=None):
            with self.mutex:
                self.count += 1
                self.inbox.append(dict(request, handle=self.count))
                self.jobs[self.count] = (chunks, done)
                if fmt is not None:
                    self.outs[self.count] = [fmt, None]
                start, self.running = not self.running, True
            if start:
                threading.Thread(target=self.work, name="tts-stream-queue", daemon=True).start()

        def take(self):
            with self.mutex:
                new, self.inbox = self.inbox, []
            return new

        def finish(self, handle, end):
            chunks, done = self.jobs.pop(handle)
            self.outs.pop(handle, None)
            chunks.put(end)
            done()

        def work(self):
            import torch
            while True:
                try:
                    with lock, torch.no_grad():
                        for handle, pcm, last in engine().serve_stream_queue(self.take, slots=int(stream_slots), **latent_kw):
                            if isinstance(pcm, BaseException):
                                self.finish(handle, pcm)
                                continue
                            out = self.outs.get(handle)
                            if out is not None:      # this request's own format: its resampler state lives as long as it does
                                if out[1] is None:
                                    out[1] = engine()._out_engine().stream(out[0])
                                pcm = out[1].push(pcm.float(), last)
                            if pcm.numel():
                                self.jobs[handle][0].put(chunk_bytes(pcm, None if out is None else out[0]))
                            if last:
                                self.finish(handle, None)
                except Exception as e:  # noqa: BLE001  (the loop itself failed: every request it had taken is told)
                    with self.mutex:
                        waiting = {r["handle"] for r in self.inbox}
                    for handle in list(self.jobs):
                        if handle not in waiting:
                            self.finish(handle, e)
                with self.mutex:
                    if not self.inbox:
                        self.running = False
                        return

    shared_loop = SharedStreamLoop()

    async def read_request(request: Request):
        """The /tts body in any of its three encodings -> (TTSRequest, uploaded prompt (filename, bytes) | None); 422 when malformed."""
        ctype = request.headers.get("content-type", "")
        body = await request.body()
        upload = None
        try:
            if ctype.startswith("application/json"):
                fields = json.loads(body or b"{}")
            elif ctype.startswith("multipart/form-data"):
                fields = _parse_multipart(body, ctype)
                up = fields.pop("prompt_audio", None)
                if isinstance(up, tuple) and up[1]:
                    upload = up
            else:
                fields = {k: v[-1] for k, v in urllib.parse.parse_qs(body.decode("utf-8")).items()}
            fields = {k: (None if isinstance(v, str) and v == "" and k in ("seed", "speaker_id", "prompt_audio_path", "sample_rate", "encoding", "pitch") + POST_FIELDS else v)
                      for k, v in fields.items()}
            return TTSRequest(**fields), upload
        except HTTPException:
            raise
        except Exception as e:  # noqa: BLE001  (validation: FastAPI answers 422 for a malformed form)
            raise HTTPException(status_code=422, detail=str(e))

    @app.post("/tts")
    async def text_to_speech(request: Request):
        req, upload = await read_request(request)
        if state["tts"] is None and not os.path.exists(model_dir):
            raise HTTPException(status_code=503, detail="the TTS engine is not initialised")
        if upload is None and not req.prompt_audio_path:
            raise HTTPException(status_code=400, detail="a reference audio is required (upload a file or give a path)")
        fmt = output_of(req)
        post = post_of(req)
        speed = speed_of(req)
        pitch = pitch_of(req)
        actual_seed = random.randint(0, 2 ** 32 - 1) if req.seed is None or req.seed == -1 else int(req.seed)
        tmp_path = None
        try:
            if upload is not None:
                suffix = os.path.splitext(upload[0] or "")[1] or ".wav"
                with tempfile.NamedTemporaryFile(delete=False, suffix=suffix) as tmp:
                    tmp.write(upload[1])
                    tmp_path = prompt = tmp.name
            else:
                if not os.path.exists(req.prompt_audio_path):
                    raise HTTPException(status_code=404, detail=f"reference audio {req.prompt_audio_path} does not exist")
                if not _inside(req.prompt_audio_path, prompt_roots):
                    raise HTTPException(status_code=403, detail="server-side prompts are only read from the prompt directory")
                prompt = req.prompt_audio_path
            os.makedirs(output_dir, exist_ok=True)
            name = f"gen_{int(time.time())}_{os.urandom(2).hex()}.wav"
            out_path = os.path.join(output_dir, name)
            kwargs = dict(do_sample=req.do_sample, top_p=req.top_p, top_k=req.top_k if req.top_k > 0 else 30,
                          temperature=req.temperature, repetition_penalty=req.repetition_penalty,
                          length_penalty=req.length_penalty, num_beams=3, max_mel_tokens=req.max_mel_tokens)
            if fmt is not None:
                kwargs["output"] = fmt
            if post is not None:
                kwargs["post"] = post
            if speed is not None:
                kwargs["speed"] = speed
            if pitch is not None:
                kwargs["pitch"] = pitch
            with lock:
                t = engine()
                set_seed(actual_seed)
                if req.infer_mode == "fast":
                    t.infer_fast(audio_prompt=prompt, text=req.text, output_path=out_path,
                                 max_text_tokens_per_sentence=req.max_text_tokens_per_sentence,
                                 sentences_bucket_max_size=req.sentences_bucket_max_size, **kwargs)
                else:
                    t.infer(audio_prompt=prompt, text=req.text, output_path=out_path,
                            max_text_tokens_per_sentence=req.max_text_tokens_per_sentence, speaker_id=req.speaker_id, **kwargs)
            if not os.path.exists(out_path):
                raise RuntimeError("no audio was produced")
            with open(out_path, "rb") as f:
                data = f.read()
            return Response(content=data, media_type="audio/wav",
                            headers={"Content-Disposition": f"attachment; filename={name}", "X-Seed": str(actual_seed)})
        except HTTPException:
            raise
        except Exception as e:  # noqa: BLE001
            raise HTTPException(status_code=500, detail=str(e))
        finally:
            if tmp_path and os.path.exists(tmp_path):
                os.remove(tmp_path)

    @app.post("/tts/stream")
    async def text_to_speech_stream(request: Request):
        """/tts's request, answered chunk by chunk while the token loop runs (IndexTTS.infer_stream): a chunked body of
        little-endian 16-bit mono PCM, audio/L16; rate=24000, header X-Seed.  Sampling runs with num_beams = 1 (a beam
        search has no final code before it ends); infer_mode, speaker_id and the bucket size do not apply.
        A worker thread takes the engine lock, runs the generation to its end and queues the chunks; the response drains the
        queue.  The lock is therefore held for the generation only -- never while progress waits for the client or the event
        loop -- and the uploaded prompt's file is removed when the worker ends, whether or not the body was read.  A request
        (of either route) that arrives during a stream waits for the lock until that generation has ended, as two /tts
        requests wait for one another; a client that reads slowly delays nobody, its chunks wait in the queue.
        The first chunk is awaited before the response starts, so what fails before it -- an unreadable prompt, a refused
        setting -- answers with /tts's status codes (500 with the error text); an error after it ends the body early."""
        req, upload = await read_request(request)
        if state["tts"] is None and not os.path.exists(model_dir):
            raise HTTPException(status_code=503, detail="the TTS engine is not initialised")
        if upload is None and not req.prompt_audio_path:
            raise HTTPException(status_code=400, detail="a reference audio is required (upload a file or give a path)")
        fmt = output_of(req)
        post_of(req, streaming=True)
        speed_of(req, streaming=True)
        pitch_of(req, streaming=True)
        actual_seed = random.randint(0, 2 ** 32 - 1) if req.seed is None or req.seed == -1 else int(req.seed)
        tmp_path = None
        if upload is not None:
            suffix = os.path.splitext(upload[0] or "")[1] or ".wav"
            with tempfile.NamedTemporaryFile(delete=False, suffix=suffix) as tmp:
                tmp.write(upload[1])
                tmp_path = prompt = tmp.name
        else:
            if not os.path.exists(req.prompt_audio_path):
                raise HTTPException(status_code=404, detail=f"reference audio {req.prompt_audio_path} does not exist")
            if not _inside(req.prompt_audio_path, prompt_roots):
                raise HTTPException(status_code=403, detail="server-side prompts are only read from the prompt directory")
            prompt = req.prompt_audio_path
        kwargs = dict(do_sample=req.do_sample, top_p=req.top_p, top_k=req.top_k if req.top_k > 0 else 30,
                      temperature=req.temperature, repetition_penalty=req.repetition_penalty,
                      length_penalty=req.length_penalty, num_beams=1, max_mel_tokens=req.max_mel_tokens, seed=actual_seed)

        chunks: "queue.Queue" = queue.Queue()     # bytes, then None (the end) or the exception that ended the generation

        def clean_up():
            if tmp_path and os.path.exists(tmp_path):
                os.remove(tmp_path)

        if stream_slots is not None:
            shared_loop.submit(dict(kwargs, audio_prompt=prompt, text=req.text,
                                    max_text_tokens_per_sentence=req.max_text_tokens_per_sentence), chunks, clean_up, fmt)
            return await respond(chunks, actual_seed, fmt)

        def work():
            import torch
            try:
                with lock, torch.no_grad():
                    for _, pcm in engine().infer_stream(prompt, req.text, req.max_text_tokens_per_sentence, **kwargs, **latent_kw,
                                                        **({} if fmt is None else {"output": fmt})):
                        chunks.put(chunk_bytes(pcm, fmt))
                chunks.put(None)
            except BaseException as e:  # noqa: BLE001  (handed to the response, which answers or ends the body)
                chunks.put(e)
            finally:
                if tmp_path and os.path.exists(tmp_path):
                    os.remove(tmp_path)

        threading.Thread(target=work, name="tts-stream", daemon=True).start()
        return await respond(chunks, actual_seed, fmt)

    async def respond(chunks, actual_seed, fmt=None):
        """The chunked answer over a queue of bytes that ends with None or an exception; the first item is awaited first."""
        first = await run_in_threadpool(chunks.get)
        if isinstance(first, HTTPException):
            raise first
        if isinstance(first, BaseException):
            raise HTTPException(status_code=500, detail=str(first))

        def body():
            item = first
            while item is not None and not isinstance(item, BaseException):
                yield item
                item = chunks.get()

        if fmt is None:
            return StreamingResponse(body(), media_type="audio/L16; rate=24000", headers={"X-Seed": str(actual_seed)})
        return StreamingResponse(body(), media_type=fmt.content_type, headers={
            "X-Seed": str(actual_seed), "X-Sample-Rate": str(fmt.sample_rate), "X-Encoding": fmt.encoding})

    return app


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="IndexTTS API server (MI355X build)")
    ap.add_argument("--host", type=str, default="127.0.0.1",
                    help="bind address (the reference binds 0.0.0.0; opt in explicitly: this server loads checkpoints)")
    ap.add_argument("--port", type=int, default=7859)
    ap.add_argument("--model_dir", type=str, default="checkpoints")
    ap.add_argument("--config", type=str, default="checkpoints/config.yaml")
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--no-fp16", action="store_true")
    ap.add_argument("--prompt_dir", type=str, default="prompts", help="directory /tts prompt_audio_path may read from")
    ap.add_argument("--stream-slots", type=int, default=None, metavar="S",
                    help="serve /tts/stream from one shared refilled loop of S decode slots (IndexTTS.stream_queue): concurrent "
                         "requests share a token loop instead of waiting for one another.  Off by default")
    ap.add_argument("--stream-latent-cache", action="store_true", default=False,
                    help="/tts/stream keeps the latent pass's keys and values between chunks (IndexTTS.infer_stream(latent_cache=True)): "
                         "a chunk boundary then costs its new rows only.  Off by default")
    ap.add_argument("--prompt-frontend", choices=("torch", "hip"), default="torch",
                    help="where a prompt's wav becomes its log-mel: torch (host ops, the default) or hip (the device front-end, "
                         "IndexTTS(prompt_frontend='hip'))")
    a = ap.parse_args()
    import uvicorn
    uvicorn.run(create_app(None, a.model_dir, a.config, a.device, not a.no_fp16, prompt_dir=a.prompt_dir, stream_slots=a.stream_slots,
                           stream_latent_cache=a.stream_latent_cache, prompt_frontend=a.prompt_frontend), host=a.host, port=a.port)
