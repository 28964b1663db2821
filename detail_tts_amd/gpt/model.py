"""UnifiedVoice mirror (reference: gpt/model.py:265-545) — device work in libdetail_hip.so (dtts_gpt_*)."""
from __future__ import annotations

import numpy as np
import torch


def _host_ints(x):
    return None if x is None else torch.as_tensor(x).detach().cpu().numpy().astype(np.int64)


def forward_inputs(text_inputs, text_lengths, mel_codes, wav_lengths, mel_length_compression=1024, stop_mel_token=8193, clip_inputs=False):
    """Host preprocessing of UnifiedVoice.forward's loss mode, in the reference's order (gpt/model.py:453-462): clip_inputs slices the
    text to text_lengths.max() columns and the codes to wav_lengths.max() // mel_length_compression; set_mel_padding (:377-390) then
    rewrites row b's codes from column wav_lengths[b] // mel_length_compression + 1 on with the stop token.  Integer arrays in,
    (text [B, Lt], codes [B, n]) int32 copies out; the inputs are left alone (the reference pads mel_codes in place)."""
    text = np.array(text_inputs, np.int64, ndmin=2)
    codes = np.array(mel_codes, np.int64, ndmin=2)
    wl = np.asarray(wav_lengths, np.int64).reshape(-1)
    if text.shape[0] != codes.shape[0] or wl.shape[0] != codes.shape[0]:
        raise ValueError(f"forward: text {text.shape}, mel_codes {codes.shape} and wav_lengths {wl.shape} disagree on the batch size")
    if clip_inputs:
        text = text[:, : int(np.asarray(text_lengths, np.int64).max())]
        codes = codes[:, : int(wl.max()) // mel_length_compression]
    for b in range(codes.shape[0]):
        end = int(wl[b]) // mel_length_compression + 1
        if end < codes.shape[1]:
            codes[b, end:] = stop_mel_token
    return np.ascontiguousarray(text, np.int32), np.ascontiguousarray(codes, np.int32)


class UnifiedVoice:
    def __init__(self, rt, cfg):
        self.rt = rt
        self.model_dim = cfg["model_dim"]
        self.max_mel_tokens = cfg["max_mel_tokens"]
        self.max_text_tokens = cfg["max_text_tokens"]
        self.start_text_token = cfg["start_text_token"]
        self.stop_text_token = 0
        self.start_mel_token = cfg["start_mel_token"]
        self.stop_mel_token = cfg["stop_mel_token"]
        self.mel_length_compression = cfg["mel_length_compression"]
        self.last_latents = None

    @staticmethod
    def _texts(text_inputs, text_lengths=None):
        t = torch.as_tensor(text_inputs).cpu().numpy().astype(np.int32)
        if t.ndim == 1:
            t = t[None]
        if text_lengths is None:
            return [r for r in t]
        tl = torch.as_tensor(text_lengths).reshape(-1).tolist()
        return [r[: int(n)] for r, n in zip(t, tl)]

    def _speaker(self, speech_conditioning_latent, cond_lengths, cond_latents):
        """-> (refer, cond): the prompt mel [B,128,T] as a contiguous fp32 tensor, or - with cond_latents [B, model_dim] - None and the
        latents.  Both given, neither, cond_lengths beside cond_latents, or a wrong width: ValueError before any launch."""
        if cond_latents is None:
            if speech_conditioning_latent is None:
                raise ValueError("neither speech_conditioning_latent (the prompt mel) nor cond_latents is given")
            return speech_conditioning_latent.float().contiguous(), None
        if speech_conditioning_latent is not None or cond_lengths is not None:
            raise ValueError("cond_latents stand in the place of speech_conditioning_latent / cond_lengths: those have to be None")
        cond = torch.as_tensor(cond_latents)
        if cond.dim() != 2 or cond.shape[1] != self.model_dim:
            raise ValueError(f"cond_latents have to be [B, {self.model_dim}], but are {tuple(cond.shape)}")
        return None, cond.to(self.rt.device, torch.float32).contiguous()

    def get_conditioning(self, speech_conditioning_input, cond_lengths=None):
        """gpt/model.py:419-427: mel [B,128,T], or n clips per speaker [B,n,128,T] -> [B, 768], the conditioning encoder's output, for n
        clips their mean (conds.mean(dim=1)): the B n clips run as one batch, then one pool launch (csrc/voice.hip).  cond_lengths
        [B] / [B,n]: every clip's valid length (an extension).  What cond_latents= takes."""
        from ..voice import check_clips
        S, n, T, lens = check_clips(speech_conditioning_input, None if speech_conditioning_input.dim() == 4 else cond_lengths,
                                    cond_lengths if speech_conditioning_input.dim() == 4 else None)
        x = speech_conditioning_input.to(self.rt.device, torch.float32).reshape(S * n, -1, T).contiguous()
        g = self.rt.mel_style("gpt.conditioning_encoder", x, lens)
        return g if n == 1 else self.rt.voice_pool(g.view(S, n, -1))

    def inference_speech_tortoise(self, speech_conditioning_latent, cond_lengths, text_inputs, input_tokens=None,
                                  num_return_sequences=1, max_generate_length=None, typical_sampling=False, typical_mass=.9,
                                  text_lengths=None, seed=0, sample_ids=None, suppress_eos=False, forced_uniforms=None, *,
                                  cond_latents=None, **hf_generate_kwargs):
        """gpt/model.py:514-545.  hf_generate_kwargs understood: do_sample, top_p, top_k, temperature, repetition_penalty, length_penalty
        (inert without beams), and HF's remaining decode-time processors, served by the device sampler in HF's order
        (gpt/decode_options.py states the counting rules): no_repeat_ngram_size (1 .. 16), min_length, min_new_tokens,
        exponential_decay_length_penalty = (start, factor > 1), suppress_tokens, begin_suppress_tokens, and - under do_sample=True only,
        as in HF - min_p and epsilon_cutoff.  Bad values raise ValueError before any launch.  `num_beams` = K in 2 .. 16 (with
        `length_penalty`, `early_stopping` in False / True / "never") runs HF's beam search on the device (csrc/gpt_beam.hip): do_sample
        has to be False or absent, `num_return_sequences` <= K then means HF's best n of the K beams, the extension keyword
        `return_scores=True` returns (sequences, sequences_scores), and last_latents is None.  Any other keyword is still dropped
        (bad_words_ids, sequence_bias, typical_p, eta_cutoff, top_h, encoder_*, group / constrained beams: INTEGRATION.md 1).  Returns LongTensor [B * num_return_sequences, <=max] incl. the stop token (and input_tokens in front).

        Off the `infer` path but part of the reference's surface: `do_sample=False` (HF greedy search: only the repetition penalty is a
        logits processor there, argmax), `num_return_sequences = n` (HF repeats every row n times - repeat_interleave - and samples the
        copies independently: `sample_ids` of length B * n name their noise streams, or of length B: copy r of row b draws from
        sample_ids[b] + r - the expanded ids must be distinct, else ValueError), `input_tokens [rows, k]` (mel tokens in front of the generated ones; with num_return_sequences = n > 1 the
        reference tiles them AND lets HF expand the batch again: n * n rows of the single prompt, reproduced), `typical_sampling`
        (HF TypicalLogitsWarper(mass=typical_mass), which HF applies between the repetition penalty and the temperature).

        cond_latents [B, 768] (here, in inference_speech_valle, forward and mel_logprobs): the conditioning encoder's output handed in -
        the role of the reference's compute_embeddings(cond_latents, text_inputs) (gpt/model.py:492-513), e.g. get_conditioning's of n
        clips or a Voice's gpt member; speech_conditioning_latent and cond_lengths are then None and the encoder is not launched."""
        return self._generate(speech_conditioning_latent, cond_lengths, text_inputs, None, input_tokens, num_return_sequences,
                              max_generate_length, typical_sampling, typical_mass, text_lengths, seed, sample_ids, suppress_eos,
                              forced_uniforms, hf_generate_kwargs, cond_latents)

    def inference_speech_valle(self, speech_conditioning_latent, cond_lengths, text_inputs, mel_codes, input_tokens=None,
                               num_return_sequences=1, max_generate_length=None, typical_sampling=False, typical_mass=.9,
                               text_lengths=None, seed=0, sample_ids=None, suppress_eos=False, forced_uniforms=None, *,
                               cond_latents=None, **hf_generate_kwargs):
        """gpt/model.py:546-579: inference_speech_tortoise continued from an acoustic prompt.  mel_codes [B, m] (or a list of B
        one-dimensional arrays: per-row lengths are an extension, the reference takes a rectangle) are mel codes in [0, 8192), e.g.
        SynthesizerTrn.encode's of a prompt mel.  Returns the GENERATED tokens only (input_tokens in front, as in tortoise); every other
        argument, num_return_sequences (prompt rows repeat as the conditioning rows do) and the extra keywords behave as there.

        Reproduced from the reference, its quirk included (gpt/prompt.py): the mel stream is [1, 8192, c_1 .. c_m] - the fill id 1 of
        the prefix columns sits at mel position 0, embedded as a mel token - and the repetition penalty starts with {1, 8192} and the
        prompt's codes.  No stop token closes the prompt (the reference keeps build_aligned_inputs_and_targets' inputs, not its
        targets), so the stop token is not in the penalty history.  The whole prompt runs in the parallel prefill; m + 3 +
        max_generate_length may not exceed the 1603 rows of mel_pos_embedding (ValueError before any launch; the reference dies with
        IndexError a little later, from m + max_generate_length = 1603).  last_latents are the hidden states with the prompt in
        context.  How a trained checkpoint sounds with a prompt is unmeasured."""
        if mel_codes is None:
            raise ValueError("inference_speech_valle: mel_codes (the acoustic prompt) is required")
        return self._generate(speech_conditioning_latent, cond_lengths, text_inputs, mel_codes, input_tokens, num_return_sequences,
                              max_generate_length, typical_sampling, typical_mass, text_lengths, seed, sample_ids, suppress_eos,
                              forced_uniforms, hf_generate_kwargs, cond_latents)

    def _generate(self, speech_conditioning_latent, cond_lengths, text_inputs, mel_codes, input_tokens, num_return_sequences,
                  max_generate_length, typical_sampling, typical_mass, text_lengths, seed, sample_ids, suppress_eos, forced_uniforms,
                  hf_generate_kwargs, cond_latents=None):
        """What inference_speech_tortoise and inference_speech_valle share (gpt/model.py:528-545 and :561-579 differ in fake_inputs only):
        the row expansion, the id checks, the greedy mapping and the decode session; mel_codes = None is the tortoise session."""
        nrs = int(num_return_sequences)
        assert nrs >= 1
        from .decode_options import validate_beam_options, validate_decode_options
        # extension keyword sampling=[...] (gpt/sampling.py): one settings dict (or None) per prompt row; a missing key takes this
        # call's own value.  The rows share the decode session, each under its own settings; with num_return_sequences they repeat.
        hf_generate_kwargs = dict(hf_generate_kwargs)
        sampling = hf_generate_kwargs.pop("sampling", None)
        # beam search (HF _beam_search, csrc/gpt_beam.hip): num_beams / length_penalty / early_stopping as the reference's
        # **hf_generate_kwargs carry them (gpt/model.py:542-544); every refusal is a ValueError before any launch
        beams, lp, es = validate_beam_options(hf_generate_kwargs.get("num_beams"), hf_generate_kwargs.get("length_penalty"),
                                              hf_generate_kwargs.get("early_stopping"), do_sample=hf_generate_kwargs.get("do_sample"),
                                              typical_sampling=typical_sampling or None, input_tokens=input_tokens,
                                              forced_uniforms=forced_uniforms, num_return_sequences=nrs)
        if beams and sampling is not None:
            raise ValueError("`sampling` cannot be combined with `num_beams` > 1 (a beam session is uniform)")
        return_scores = bool(hf_generate_kwargs.get("return_scores", False))
        if return_scores and not beams:
            raise ValueError("`return_scores` needs `num_beams` > 1 (sequences_scores are a beam search's)")
        do_sample = False if beams else bool(hf_generate_kwargs.get("do_sample", True))
        processors = validate_decode_options({k: v for k, v in hf_generate_kwargs.items() if k not in ("num_beams", "length_penalty", "early_stopping")},
                                             do_sample=do_sample, strict=False)      # (ValueError before any launch)
        refer, cond = self._speaker(speech_conditioning_latent, cond_lengths, cond_latents)      # (ValueError before any launch)
        dev = (refer if cond is None else cond).device
        if beams:
            B = (refer if cond is None else cond).shape[0]
            cl = None if cond_lengths is None else torch.as_tensor(cond_lengths).reshape(-1).tolist()
            prompt = None
            if mel_codes is not None:
                from .prompt import prompt_rows
                prompt = prompt_rows(mel_codes, B)
            G = self.max_mel_tokens - 1 if max_generate_length is None else int(max_generate_length)
            seqs, lens, scores = self.rt.gpt_generate_beams(
                refer, cl, self._texts(text_inputs, text_lengths), beams, num_return_sequences=nrs, max_generate_length=G, length_penalty=lp,
                early_stopping={0: False, 1: True, 2: "never"}[es], repetition_penalty=hf_generate_kwargs.get("repetition_penalty", 1.0),
                suppress_eos=suppress_eos, prompt_codes=prompt, processors=processors or None, cond=cond)
            # rows change lineage while decoding: no decode-time latents (forward(return_latent=True) on the chosen codes gives them)
            self.last_latents, self.last_ncodes = None, lens.reshape(-1)
            self.last_scores = torch.from_numpy(scores.reshape(-1).copy())
            out = torch.from_numpy(seqs.reshape(B * nrs, G)[:, :int(lens.max())].astype(np.int64)).to(dev)
            return (out, self.last_scores) if return_scores else out
        B = (refer if cond is None else cond).shape[0]
        rows = None
        if sampling is not None:        # (ValueError before any launch)
            from .sampling import repeat_rows, resolve_sampling
            G0 = self.max_mel_tokens - 1 if max_generate_length is None else int(max_generate_length)
            greedy = not do_sample
            rows = resolve_sampling(sampling, B, top_k=1 if greedy else int(hf_generate_kwargs.get("top_k", 50) or 0), max_generate_length=G0,
                                    decode_options=processors, num_beams=beams or None, always_rows=True,
                                    base=dict(temperature=1.0 if greedy else hf_generate_kwargs.get("temperature", 1.0),
                                              top_p=1.0 if greedy else hf_generate_kwargs.get("top_p", 1.0),
                                              repetition_penalty=hf_generate_kwargs.get("repetition_penalty", 1.0),
                                              typical_mass=float(typical_mass) if typical_sampling else 0.0))
            rows = repeat_rows(rows, nrs if input_tokens is None or nrs == 1 else nrs * nrs)
        it = None
        if input_tokens is not None:
            it = torch.as_tensor(input_tokens).cpu().numpy().astype(np.int32)
            assert it.ndim == 2
            if nrs > 1:
                # gpt/model.py:533-537: the reference tiles the prompt's fake inputs n times and the prefixes n // rows times (its torch.cat
                # needs n * B == n rows: ONE prompt), then HF's generate expands every row n times again (repeat_interleave): n * n returned
                # rows, row r starting with input_tokens[(r // n) % rows] and sampling from its own stream
                assert nrs % it.shape[0] == 0, "The number of return sequences must be divisible by the number of input sequences"
                if B != 1:
                    raise ValueError("input_tokens with num_return_sequences > 1: the reference concatenates num_return_sequences * B rows of "
                                     "inputs with num_return_sequences rows of prefixes - a single prompt only")
                it = np.stack([it[(r // nrs) % it.shape[0]] for r in range(nrs * nrs)])
                nrs = nrs * nrs
        cl = None if cond_lengths is None else torch.as_tensor(cond_lengths).reshape(-1).tolist()
        texts = self._texts(text_inputs, text_lengths)
        prompt = None
        if mel_codes is not None:
            from .prompt import prompt_rows
            prompt = prompt_rows(mel_codes, B)
        ids = list(range(B * nrs)) if sample_ids is None else list(sample_ids)
        if nrs > 1:
            refer = None if refer is None else refer.repeat_interleave(nrs, 0).contiguous()
            cond = None if cond is None else cond.repeat_interleave(nrs, 0).contiguous()
            cl = None if cl is None else [v for v in cl for _ in range(nrs)]
            texts = [t for t in texts for _ in range(nrs)]
            prompt = None if prompt is None else [p for p in prompt for _ in range(nrs)]
            if len(ids) == B:
                ids = [i + r for i in ids for r in range(nrs)]
        assert len(ids) == B * nrs, "sample_ids: one per returned sequence (or one per prompt)"
        if len(set(ids)) != len(ids):
            # HF samples all copies independently: two returned sequences on ONE Philox stream would be the same draw sequence
            # (per-prompt ids [0, 1] with n = 2 expand to [0, 1, 1, 2]: ADVICE r05)
            raise ValueError(f"sample_ids expand to {ids}: two returned sequences would share a noise stream - pass B * num_return_sequences "
                             "distinct ids (or per-prompt ids at least num_return_sequences apart)")
        G = self.max_mel_tokens - 1 if max_generate_length is None else int(max_generate_length)
        forced = None
        if it is not None:
            assert it.shape[0] == B * nrs and it.shape[1] <= G
            forced = [row for row in it]
        if do_sample:
            samp = dict(top_k=hf_generate_kwargs.get("top_k", 50), top_p=hf_generate_kwargs.get("top_p", 1.0),
                        temperature=hf_generate_kwargs.get("temperature", 1.0))
        else:       # greedy search = the one largest logit after the repetition penalty: top-k 1 keeps exactly it (any draw picks it)
            samp = dict(top_k=1, top_p=1.0, temperature=1.0)
        if rows is not None:
            from .sampling import session_cap
            Gs = session_cap(rows, G)
            if Gs != G and forced_uniforms is not None:       # (its row stride is the call's max_generate_length)
                raise ValueError(f"sampling: every row's `max_generate_length` is below the call's {G}, which `forced_uniforms` is shaped "
                                 "for - keep one row at the call's length")
            if forced is not None and max(len(row) for row in forced) > Gs:
                raise ValueError(f"sampling: `input_tokens` are longer than the largest row cap {Gs}")
            G = Gs
        codes, ncodes, lat = self.rt.gpt_generate(
            refer, cl, texts, seed, ids, max_generate_length=G, repetition_penalty=hf_generate_kwargs.get("repetition_penalty", 1.0),
            suppress_eos=suppress_eos, forced_uniforms=forced_uniforms, forced_codes=forced, forced_fill=-1,
            typical_mass=float(typical_mass) if typical_sampling else 0.0, **samp, **({} if prompt is None else dict(prompt_codes=prompt)),
            **({"processors": processors} if processors else {}), cond=cond, rows=rows)
        self.last_latents, self.last_ncodes = lat, ncodes
        n = int(ncodes.max())
        return torch.from_numpy(codes[:, :n].astype(np.int64)).to(dev)

    def forward(self, speech_conditioning_latent, cond_lengths, text_inputs, text_lengths, mel_codes, wav_lengths, types=None,
                text_first=True, raw_mels=None, return_attentions=False, return_latent=False, clip_inputs=False, *, return_logits=True,
                cond_latents=None):
        """gpt/model.py:429-491.

        return_latent=True (the inference use, vqvae/model_24k.py:796-799) -> latents [B, n, 768]; rows are ragged there (text_lengths
        and wav_lengths give every row its own length).

        Otherwise the reference's loss mode -> (loss_text, loss_mel, mel_logits): two 0-d fp32 CUDA tensors and [B, 8194, n + 2]
        (None with return_logits=False: no logits are materialised).  The batch is the reference's RECTANGLE: its forward has no
        attention mask and takes both cross-entropies as plain means over all B (Lt + 2) / B (n + 2) positions, so every row counts with
        the full text_inputs.shape[1] and mel_codes.shape[1]; text_lengths matters only under clip_inputs, wav_lengths only through
        clip_inputs and set_mel_padding (forward_inputs).  Needs gpt.text_head in the checkpoint (dtts_gpt_forward_losses)."""
        if types is not None or raw_mels is not None or not text_first or (return_attentions and not return_latent):
            raise NotImplementedError("UnifiedVoice.forward: types, raw_mels, text_first=False and return_attentions=True are not implemented "
                                      "on the device")
        refer, cond = self._speaker(speech_conditioning_latent, cond_lengths, cond_latents)
        if not return_latent:
            cl = None if cond_lengths is None else torch.as_tensor(cond_lengths).reshape(-1).tolist()
            text, codes = forward_inputs(_host_ints(text_inputs), _host_ints(text_lengths), _host_ints(mel_codes), _host_ints(wav_lengths),
                                         self.mel_length_compression, self.stop_mel_token, clip_inputs)
            losses, logits = self.rt.gpt_forward_losses(refer, cl, text, codes, want_logits=bool(return_logits), cond=cond)
            return losses[0], losses[1], logits
        cl = None if cond_lengths is None else torch.as_tensor(cond_lengths).reshape(-1).tolist()
        codes = torch.as_tensor(mel_codes).cpu().numpy().astype(np.int32)
        wl = torch.as_tensor(wav_lengths).reshape(-1).tolist()
        code_list = []
        for b in range(codes.shape[0]):
            row = codes[b].copy()
            end = int(wl[b]) // self.mel_length_compression + 1            # set_mel_padding, gpt/model.py:377-390
            if end < row.shape[-1]:
                row[end:] = self.stop_mel_token
            code_list.append(row)
        lat = self.rt.gpt_latents(refer, cl, self._texts(text_inputs, text_lengths), code_list, cond=cond)
        return lat.permute(0, 2, 1).contiguous()

    def mel_logprobs(self, speech_conditioning_latent, cond_lengths, text_inputs, text_lengths, mel_codes_list, *, cond_latents=None):
        """Teacher-forced log-probabilities: for every row the fp32 numpy array log p(c_k | prompt, c_1 .. c_{k-1}), k = 1 .. n, of its
        codes c_1 .. c_n under the model's unprocessed distribution = log_softmax(mel_logits)[c_k] of the reference's forward
        (gpt/model.py:408-415, 479) at the positions of the codes.  Rows may differ in length; append the stop token (8193) to a row to
        score its stop as well.  Runs rt.gpt_latents, then rt.gpt_score on those latents (no [B, V, n] logits are materialised)."""
        refer, cond = self._speaker(speech_conditioning_latent, cond_lengths, cond_latents)
        cl = None if cond_lengths is None else torch.as_tensor(cond_lengths).reshape(-1).tolist()
        codes = [np.asarray(torch.as_tensor(c).cpu().numpy() if not isinstance(c, np.ndarray) else c, np.int32).reshape(-1) for c in mel_codes_list]
        lat = self.rt.gpt_latents(refer, cl, self._texts(text_inputs, text_lengths), codes, cond=cond)
        lp = self.rt.gpt_score(lat, codes).cpu().numpy()
        return [lp[b, : len(c)].copy() for b, c in enumerate(codes)]

    @staticmethod
    def _code_rows(mel_codes):
        """[B, n] (tensor / array) or a list of B one-dimensional rows -> list of int32 arrays"""
        if isinstance(mel_codes, (list, tuple)):
            return [np.asarray(torch.as_tensor(c).cpu().numpy() if not isinstance(c, np.ndarray) else c, np.int32).reshape(-1) for c in mel_codes]
        c = torch.as_tensor(mel_codes).cpu().numpy().astype(np.int32)
        return [r for r in (c[None] if c.ndim == 1 else c)]

    def attentions(self, speech_conditioning_latent, cond_lengths, text_inputs, mel_codes, *, text_lengths=None, layers=None,
                   cond_latents=None):
        """The GPT's attention maps of the teacher-forced pass over [cond | 255, text, 0 | 8192, codes, 8193]: a tuple of [B, 16, L, L]
        CUDA tensors, one per selected layer (`layers`: distinct ids, None = all 10) - the value of the reference's
        get_logits(..., get_attns=True) (gpt/model.py:392-400).  forward(return_attentions=True) keeps refusing: the reference's own
        unpacks the 10-tuple into two names and fails, so there is no value of it to mirror.  Rows may be ragged (text_lengths, a list
        of code rows): row b fills its own top-left lt_b x lt_b, lt_b = 1 + (text_b + 2) + (codes_b + 2), the rest is 0.  A result
        above 1 GiB raises ValueError naming `layers`.  One extra kernel per selected layer (csrc/attn_probs.hip) in the pass that
        forward(return_latent=True) runs; exact-fp32 scores."""
        refer, cond = self._speaker(speech_conditioning_latent, cond_lengths, cond_latents)
        cl = None if cond_lengths is None else torch.as_tensor(cond_lengths).reshape(-1).tolist()
        out = self.rt.gpt_attentions(refer, cl, self._texts(text_inputs, text_lengths), self._code_rows(mel_codes), layers=layers, cond=cond)
        return tuple(out[k] for k in range(out.shape[0]))

    def text_alignment(self, speech_conditioning_latent, cond_lengths, text_inputs, text_lengths, mel_codes_list, *, layers=None,
                       head_weights=None, cond_latents=None):
        """Which text column every mel code sits on, from the text-audio attention of the teacher-forced pass:
        dict(attn cuda [B, n_max, tl_max], text_mass cuda [B, n_max], path cuda int32 [B, n_max]).  attn[b, j, i] is the attention of
        the column that PREDICTS code j (the start-mel column for code 0) to text column i of [255, text, 0], summed over the selected
        `layers` and the 16 heads with `head_weights` [len(layers), 16] (None: the uniform mean); its softmax ran over ALL keys, so
        text_mass = attn.sum(-1) says how much sits on the text at all.  path is the monotone path of largest total
        log(clamp_min(attn, 1e-12)) (csrc/align_path.hip; -1 beyond a row's codes): it may stay on a column or jump ahead.  Which
        layers and heads carry the alignment of a trained checkpoint is unknown here, and alignment quality is unmeasured."""
        refer, cond = self._speaker(speech_conditioning_latent, cond_lengths, cond_latents)
        cl = None if cond_lengths is None else torch.as_tensor(cond_lengths).reshape(-1).tolist()
        texts, codes = self._texts(text_inputs, text_lengths), self._code_rows(mel_codes_list)
        attn, mass = self.rt.gpt_text_alignment(refer, cl, texts, codes, layers=layers, head_weights=head_weights, cond=cond)
        path = self.rt.op_monotone_path(torch.log(attn.clamp_min(1e-12)), [len(c) for c in codes], [len(t) + 2 for t in texts])
        return dict(attn=attn, text_mass=mass, path=path)

    __call__ = forward
