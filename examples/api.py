#!/usr/bin/env python3
"""The reference's api.py flow (api.py:10-50) on the MI355X path: reference wav -> resample -> log-mel -> GPT codes -> diffusion ->
vocoder -> gen.wav.  Everything after reading the file runs in libdetail_hip.so.

    python examples/api.py --ckpt /path/model-480.pt --vocab /path/bpe_tokenizers/zh_tokenizer.json --wav 1.wav \\
        --text "da4 jia1 hao3 ， jin1 tian1 lai2 dian3 da4 jia1 xiang3 kan4 de5 dong1 xi1 。"
    python examples/api.py --synthetic            # no checkpoint / vocabulary: seed-0 random weights, random ids, a synthetic prompt
    python examples/api.py --ckpt ... --vocab ... --wav 1.wav --text-file chapter.txt     # a long pinyin text: infer_long, one wav
"""
import argparse
import os
import sys
import wave

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from detail_tts_amd.prepare.load_infer import load_model                                    # api.py:27
from detail_tts_amd.vqvae.model_24k import write_wav
from detail_tts_amd.vqvae.utils.data_utils import HParams, Resample, load_config, mel_spectrogram_torch   # api.py:29


def read_wav(path):
    with wave.open(path, "rb") as f:
        sr, n, ch, sw = f.getframerate(), f.getnframes(), f.getnchannels(), f.getsampwidth()
        pcm = np.frombuffer(f.readframes(n), {1: np.uint8, 2: np.int16, 4: np.int32}[sw]).reshape(-1, ch)
    scale = {1: 128.0, 2: 32768.0, 4: 2147483648.0}[sw]
    x = (pcm.astype(np.float32) - (128.0 if sw == 1 else 0.0)) / scale
    return torch.from_numpy(x.T[:1].copy()), sr                                           # first channel (api.py:36-37)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", default="synthetic:0")
    ap.add_argument("--vocab")
    ap.add_argument("--wav")
    ap.add_argument("--text", "--pinyin", dest="text", default="da4 jia1 hao3",
                    help="the sentence AS PINYIN (pypinyin Style.TONE3, neutral tone 5, space separated: what api.py:21 produces from "
                         "Chinese characters; pypinyin's dictionary is not available offline, so the conversion is the caller's)")
    ap.add_argument("--print-ids", action="store_true", help="print the text token ids as JSON and exit (no GPU needed)")
    ap.add_argument("--ids", help="comma-separated text token ids (bypasses pypinyin + tokenizer: e.g. the demo.ipynb KAT ids)")
    ap.add_argument("--seed", type=int)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--out", default="gen.wav")
    ap.add_argument("--max-generate-length", type=int, default=600)
    ap.add_argument("--save-voice", metavar="FILE", help="write the prompt's conditioning latents (a Voice, one .npz) and synthesise with them")
    ap.add_argument("--voice", metavar="FILE", help="synthesise with a stored Voice: no prompt wav is read and no prompt encoder runs")
    ap.add_argument("--timings", metavar="PATH", help="also align the synthesised codes to the text (infer(return_alignment=True)) and write "
                                                      "the token and word spans and times as JSON; words need --vocab (its [SPACE] id)")
    ap.add_argument("--text-file", metavar="PATH", help="a text of any length AS PINYIN: split at sentence ends, synthesised chunk by chunk "
                                                        "and joined into one wav (infer_long); without --vocab a character stands for an id")
    ap.add_argument("--pause-ms", type=float, nargs=4, metavar=("SENTENCE", "CLAUSE", "WORD", "HARD"),
                    help="with --text-file: the silence behind a chunk by how it ended (default 400 200 60 0; unmeasured under a trained checkpoint)")
    ap.add_argument("--max-len", type=int, default=160, help="with --text-file: the most characters of a chunk")
    ap.add_argument("--speed", type=float, help="the speaking rate, 0.25 .. 4.0 (infer(speed=) / infer_long(speed=): 0.8 is slower, 1.25 faster; "
                                                "audio quality at other rates is unmeasured under a trained checkpoint)")
    ap.add_argument("--temperature", type=float, help="stage A's sampling temperature (infer(sampling=dict(temperature=)); default 0.8)")
    ap.add_argument("--top-p", type=float, help="stage A's nucleus mass in (0, 1] (default 0.8)")
    ap.add_argument("--repetition-penalty", type=float, help="stage A's repetition penalty (default 2.0); how any of the three sounds "
                                                             "under a trained checkpoint is unmeasured")
    a = ap.parse_args()
    sampling = {k: v for k, v in (("temperature", a.temperature), ("top_p", a.top_p), ("repetition_penalty", a.repetition_penalty)) if v is not None}
    if a.voice and (a.wav or a.save_voice):
        ap.error("--voice stands in the place of the prompt: not with --wav or --save-voice")
    if a.text_file and a.timings:
        ap.error("--timings is not available with --text-file: word timings across chunks are not implemented "
                 "(infer_long(return_chunks=True) gives every chunk's offset)")
    if a.text_file and (a.ids or a.print_ids):
        ap.error("--text-file takes the text from the file: not with --ids or --print-ids")
    if (a.pause_ms or a.max_len != 160) and not a.text_file:
        ap.error("--pause-ms and --max-len belong to --text-file")
    device = "cuda:0"
    if a.ids:
        ids = [int(v) for v in a.ids.split(",")]
    elif a.vocab:
        from detail_tts_amd.bpe_tokenizers.voice_tokenizer import VoiceBpeTokenizer
        ids = VoiceBpeTokenizer(a.vocab).encode(" " + a.text.strip() + " ")                 # api.py:22-24
    else:
        ids = np.random.RandomState(0).randint(3, 255, 24).tolist()
    if a.print_ids:
        import json
        print(json.dumps(ids))
        return
    text_tokens = F.pad(torch.IntTensor(ids).unsqueeze(0), (0, 1))                          # api.py:24-25
    vqvae = load_model("vqvae", a.ckpt, None, device)                                       # api.py:33
    text_lengths = torch.LongTensor([text_tokens.shape[-1]])
    kw = dict(max_generate_length=a.max_generate_length, seed=a.seed, suppress_eos=a.synthetic or a.ckpt.startswith("synthetic"))
    if a.speed is not None:
        kw.update(speed=a.speed)
    if sampling:
        kw.update(sampling=sampling)
    if a.timings:
        space = None
        if a.vocab and not a.ids:
            space = VoiceBpeTokenizer(a.vocab).tokenizer.token_to_id("[SPACE]")
        kw.update(return_alignment=True, align_options=dict(space_id=space))

    def finish(result):
        """the waveform of an infer call; with --timings its alignment goes to the JSON file"""
        if not a.timings:
            return result
        import json
        wav, (al,) = result
        doc = dict(ids=[int(v) for v in text_tokens[0].tolist()], sampling_rate=24000, stats=al["stats"],
                   tokens=[dict(index=k, id=int(text_tokens[0, k]), codes=s, seconds=t) for k, (s, t) in enumerate(zip(al["token_spans"], al["token_times"]))],
                   words=[dict(tokens=w["tokens"], codes=w["span"], seconds=w["time"]) for w in al.get("words", [])])
        with open(a.timings, "w") as f:
            json.dump(doc, f, indent=1)
        print(f"{a.timings}: {len(doc['tokens'])} tokens, {len(doc['words'])} words, coverage {al['stats']['coverage']:.2f} "
              "(alignment quality is unmeasured: no trained checkpoint)")
        return wav
    if a.text_file:
        a.long = dict(text=open(a.text_file, encoding="utf-8").read(), max_len=a.max_len, seed=a.seed, suppress_eos=kw["suppress_eos"],
                      max_generate_length=a.max_generate_length, speed=a.speed, sampling=sampling or None)
        if a.pause_ms:
            a.long["pauses_ms"] = dict(zip(("sentence", "clause", "word", "hard"), a.pause_ms))
        if a.vocab:
            a.long["tokenizer"] = VoiceBpeTokenizer(a.vocab)
        else:       # no vocabulary: a character stands for an id (synthetic weights only - the ids mean nothing)
            a.long["tokenizer"] = type("CharIds", (), dict(encode=staticmethod(lambda t: [3 + ord(c) % 250 for c in t])))()

    def long_form(**speaker):
        """--text-file: the whole text through infer_long in the prompt's voice -> the wav file"""
        with torch.no_grad():
            wav, chunks = vqvae.infer_long(a.long.pop("text"), return_chunks=True, **speaker, **a.long)
        write_wav(a.out, wav.squeeze(0), 24000)
        cut = sum(c["codes"] is not None and c["codes"] >= a.max_generate_length - 1 for c in chunks)      # (None under --speed)
        print(f"{a.out}: {wav.shape[-1] / 24000:.2f} s of audio from {len(chunks)} chunks of {a.text_file}"
              + (f"; {cut} chunks ran into --max-generate-length and were cut short" if cut and not kw["suppress_eos"] else ""))

    if a.voice:
        from detail_tts_amd.voice import Voice
        if a.text_file:
            return long_form(speaker=Voice.load(a.voice, vqvae))
        with torch.no_grad():
            wav = finish(vqvae.infer(text_tokens, text_lengths, None, None, speaker=Voice.load(a.voice, vqvae), **kw))
        write_wav(a.out, wav.squeeze(0), 24000)
        print(f"{a.out}: {wav.shape[-1] / 24000:.2f} s of audio in the voice of {a.voice} from {len(ids)} text ids")
        return
    if a.wav:
        audio, sr = read_wav(a.wav)                                                         # api.py:34-37
    else:
        sr = 44100
        t = torch.arange(3 * sr) / sr
        audio = (0.2 * torch.sin(2 * np.pi * 220 * t) * torch.exp(-t) + 0.02 * torch.randn(3 * sr))[None]
    audio = Resample(sr, 24000, rt=vqvae.rt)(audio)                                         # api.py:39
    hps = HParams(**load_config())
    spec = mel_spectrogram_torch(audio, hps.data.filter_length, hps.data.n_mel_channels, hps.data.sampling_rate, hps.data.hop_length,
                                 hps.data.win_length, hps.data.mel_fmin, hps.data.mel_fmax, rt=vqvae.rt)      # api.py:41-47
    spec_lengths = torch.LongTensor([spec.shape[-1]])
    if a.text_file:
        with torch.no_grad():
            voice = vqvae.get_conditioning_latents(spec, spec_lengths)
        if a.save_voice:
            voice.save(a.save_voice)
        return long_form(speaker=voice)
    with torch.no_grad():
        if a.save_voice:        # the prompt is encoded once, here; --voice FILE reuses it (the same waveform bit for bit)
            voice = vqvae.get_conditioning_latents(spec, spec_lengths)
            voice.save(a.save_voice)
            wav = finish(vqvae.infer(text_tokens, text_lengths, None, None, speaker=voice, **kw))
        else:
            wav = finish(vqvae.infer(text_tokens, text_lengths, spec, spec_lengths, **kw))     # api.py:49
    write_wav(a.out, wav.squeeze(0), 24000)                                                  # api.py:50
    print(f"{a.out}: {wav.shape[-1] / 24000:.2f} s of audio from {spec.shape[-1]} prompt frames and {len(ids)} text ids")


if __name__ == "__main__":
    main()
