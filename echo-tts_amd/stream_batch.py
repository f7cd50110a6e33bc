"""Continuous batching for blockwise streaming: streams that arrived at different times share one sampler call per block.

The reference generates an utterance block by block (inference_blockwise.py:59-121): block k is one Euler run of `block_size` latents at
start_pos = the latents generated so far, attending to the latent-prefix KV of what exists.  `sample_blockwise_stream` does that for the
rows of ONE request batch, which move in lockstep.  Streaming clients never arrive together, so a server with eight open streams ran eight
batch-1 samplers.  `StreamBatcher` keeps the open streams and runs, per `step()`, one `echo_sample_euler_items_pos` call for up to
`max_batch` of them: every row brings its own start position, request parameters and cached voice.

What is rebuilt per call (stated, measured by tools/bench_stream_batch.py): the text KV of the call's rows and the latent-prefix KV of their
stacked prefixes (one encode up to the longest prefix; the latent encoder is causal, shorter items are masked by key count and their rows
are zero beyond their own prefix); the voices are bound from their captured caches (`EchoDiT.bind_voices`), not re-encoded.

Mixed block sizes (`StreamBatcher(mix_block_sizes=True)`, `plan_stream_step_mixed`): a call is then keyed by `num_steps` alone and runs at
the largest block size among its streams; a shorter block rides along as a padded row with its own length (`echo_sample_euler_items_len`).
`max_pad_fraction` bounds the share of padded tokens a call may carry.

Batched decode (`StreamBatcher(batch_decode=True)`): `step_audio()` hands the step's new blocks to ONE `DACStream.push_many` call
(`echo_dac_decode_tail_items`: the tails of all streams share the decoder front and every convolution launch) instead of one `push` per
stream; continuation prefixes are pushed first, in one call of their own.  Off by default (DESIGN.md 3.13 has the measured A/B).

Mixed step counts (`StreamBatcher(mix_block_sizes=True, mix_steps=True)`): a call's key is then empty - streams of any `num_steps` share it,
each running its own number of steps (`echo_sample_euler_items_steps`); a stream that finishes early rides along to the
call's last step.  `max_idle_fraction` bounds the share of such idle (stream, step) pairs a call may carry.  Off by default.

Not here: a captured text KV, incremental prefix encoding, dropping a finished stream from a running call."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import torch

from .model import MAX_ITEMS

# the per-request sampler keys of a stream: inference.ITEM_KEYS without the seed (noise is drawn per stream from `rng_seed`)
STREAM_ITEM_KEYS = ("num_steps", "cfg_scale_text", "cfg_scale_speaker", "cfg_min_t", "cfg_max_t", "truncation_factor", "rescale_k",
                    "rescale_sigma", "speaker_kv_scale", "speaker_kv_max_layers", "speaker_kv_min_t")
_NO_VOICE = "\0no-voice"      # the one-masked-key voice of a stream without a speaker (inference.py:341-346), as handler.synthesize_many


@dataclass
class StreamState:
    """What the planner needs to know of one open stream (pure host data), plus the device state `StreamBatcher` hangs on it."""
    id: int
    arrival: int                       # order of `open` calls
    block_sizes: Tuple[int, ...]
    num_steps: int
    next_block: int = 0
    waiting_since: int = 0             # the step counter's value when the stream was opened or last got a block
    # ---- device side (unused by plan_stream_step)
    item: Optional[dict] = None
    ids: Optional[torch.Tensor] = None
    tmask: Optional[torch.Tensor] = None
    voice: object = None
    prefix: Optional[torch.Tensor] = None      # (P, latent) fp32: continuation + every block, zero where nothing was generated yet
    start: int = 0
    x_inits: Optional[list] = None
    rng: object = None
    dec: object = None
    extra: dict = field(default_factory=dict)

    @property
    def finished(self) -> bool:
        return self.next_block >= len(self.block_sizes)

    @property
    def key(self) -> Optional[Tuple[int, int]]:
        """(block_size, num_steps) of the next block: the two things one sampler call cannot mix (they set the launch geometry)."""
        return None if self.finished else (int(self.block_sizes[self.next_block]), int(self.num_steps))


def plan_stream_step(states: Sequence[StreamState], max_batch: int) -> List[int]:
    """Which streams the next sampler call carries: the ids, leader first.  Pure function of the states.

    The leader is the stream that has waited longest (smallest `waiting_since`, ties by arrival): a stream that was skipped - other block
    size, other step count, or no room - is therefore first the next time.  The call is then filled, in arrival order, with up to `max_batch`
    open streams whose next block has the leader's (block_size, num_steps).  A finished stream takes no row.  [] when nothing waits."""
    cap = max(1, min(int(max_batch), MAX_ITEMS))
    open_ = [s for s in states if not s.finished]
    if not open_:
        return []
    leader = min(open_, key=lambda s: (s.waiting_since, s.arrival))
    rest = sorted((s for s in open_ if s is not leader and s.key == leader.key), key=lambda s: s.arrival)
    return [leader.id] + [s.id for s in rest[:cap - 1]]


def padded_share(block_sizes: Sequence[int]) -> float:
    """sum(S_call - b_i) / (n * S_call) of one call, S_call = the largest block size in it: the share of its token rows that is padding."""
    n, s_call = len(block_sizes), max(int(b) for b in block_sizes)
    return sum(s_call - int(b) for b in block_sizes) / float(n * s_call)


def idle_share(step_counts: Sequence[int], compact: bool = False) -> float:
    """sum(N - n_i) / (n * N) of one call, N = the largest step count in it: the share of its (stream, iteration) pairs in which a stream
    has already finished and only rides along.  `compact=True` (a call with compacted row sets): a finished stream has no
    rows, nothing rides along: 0."""
    if compact:
        return 0.0
    n, top = len(step_counts), max(int(v) for v in step_counts)
    return sum(top - int(v) for v in step_counts) / float(n * top)


def plan_stream_step_mixed(states: Sequence[StreamState], max_batch: int, max_pad_fraction: Optional[float] = None, mix_steps: bool = False,
                           max_idle_fraction: Optional[float] = None, compact: bool = False) -> List[int]:
    """`plan_stream_step` for calls that mix block sizes: the key of a call is `num_steps` alone.  Pure function of the states.

    The leader is chosen as there (longest wait, ties by arrival).  The call is filled in arrival order with open streams of the leader's
    `num_steps`; a candidate is skipped when taking it would raise the call's padded share (`padded_share` of the block sizes taken so far
    plus its own) above `max_pad_fraction` (None: no limit).  A skipped stream keeps its `waiting_since` and so leads sooner the next time.

    `mix_steps=True`: the key of a call is empty - every open stream is a candidate whatever its `num_steps`.  Leader rule and arrival order
    are unchanged; a candidate is also skipped when taking it would raise the call's idle share (`idle_share` of the step counts taken so far
    plus its own) above `max_idle_fraction` (None: no limit).  `compact=True`: the calls compact their row sets (`idle_share(compact=True)`
    is 0), so the idle limit skips nobody."""
    cap = max(1, min(int(max_batch), MAX_ITEMS))
    open_ = [s for s in states if not s.finished]
    if not open_:
        return []
    leader = min(open_, key=lambda s: (s.waiting_since, s.arrival))
    picked, sizes, counts = [leader.id], [leader.key[0]], [int(leader.num_steps)]
    for s in sorted((s for s in open_ if s is not leader and (mix_steps or int(s.num_steps) == int(leader.num_steps))), key=lambda s: s.arrival):
        if len(picked) >= cap:
            break
        if max_pad_fraction is not None and padded_share(sizes + [s.key[0]]) > float(max_pad_fraction):
            continue
        if mix_steps and max_idle_fraction is not None and idle_share(counts + [int(s.num_steps)], compact) > float(max_idle_fraction):
            continue
        picked.append(s.id)
        sizes.append(s.key[0])
        counts.append(int(s.num_steps))
    return picked


def schedule_ts(num_steps: int) -> torch.Tensor:
    return torch.linspace(1.0, 0.0, int(num_steps) + 1) * 0.999          # inference.py:452,459


def check_stream_request(item: dict, block_sizes: Sequence[int], continuation_len: int, max_pos: int) -> None:
    """The stated limits of a stream, each a ValueError with its reason.  Host only; runs before any device work."""
    unknown, missing = set(item) - set(STREAM_ITEM_KEYS), set(STREAM_ITEM_KEYS) - set(item)
    if unknown or missing:
        raise ValueError(f"stream parameters: unknown keys {sorted(unknown)}, missing keys {sorted(missing)}")
    if not block_sizes or any(int(b) < 1 for b in block_sizes):
        raise ValueError("block_sizes must name at least one block of at least one latent")
    if item["speaker_kv_scale"] is not None:
        # inference_blockwise.py:68-70 multiplies the ONE persistent speaker cache at the start of every block; inference.py:511-513 divides it
        # again only at the step that crosses speaker_kv_min_t.  Without such a step the factor compounds block after block.  A batched call
        # binds every voice fresh from its captured cache and scales it once: it can reproduce "scaled, then undone inside the block" only.
        ts, mt = schedule_ts(item["num_steps"]), item["speaker_kv_min_t"]
        undone = mt is not None and any(bool(ts[i + 1] < mt) and bool(ts[i] >= mt) for i in range(int(item["num_steps"])))
        if not undone:
            raise ValueError("speaker_kv_scale without a step that crosses speaker_kv_min_t: the speaker-KV scale is never undone inside a block, "
                             "the reference then compounds the factor block after block on one persistent cache, and a cache bound fresh "
                             "per call cannot reproduce that")
    total = int(continuation_len) + sum(int(b) for b in block_sizes)
    if total > max_pos:
        raise ValueError(f"continuation_latent of {int(continuation_len)} latents plus {total - int(continuation_len)} to generate needs "
                         f"{total} positions: longer than the RoPE table allows ({max_pos})")


class StreamBatcher:
    """Open streams share sampler calls.  `open()` registers a stream, `step()` runs one call for the streams `plan_stream_step` picks and
    returns their new blocks, `step_audio()` also decodes them (one `DACStream` per stream).  Single-threaded, like the context it drives.

    `voices`: a `handler.VoiceCache`, or a dict name -> (speaker_latent, speaker_mask) or 44.1 kHz audio (1, n), as
    `handler.synthesize_many` takes it.  `open(speaker_voice=)` names one, passes a captured batch-1 `VoiceHandle`, or None (no speaker).

    `mix_block_sizes=True`: streams whose next blocks differ in size share a call (`plan_stream_step_mixed`, bounded by `max_pad_fraction`);
    the default keeps one call per (block_size, num_steps).

    `batch_decode=True`: `step_audio()` decodes the step's blocks in one `DACStream.push_many` call instead of one `push` per stream.

    `mix_steps=True` (needs `mix_block_sizes=True`: ValueError otherwise): streams with different `num_steps` share a call too, bounded by
    `max_idle_fraction`; the call's rows are ordered by step count, longest first, and `stats["idle_steps"]` counts the ride-along steps.

    `compact_rows=True` (default off): every sampler call runs only the rows somebody reads (`run_euler_items(compact_rows=True)`):
    a finished stream has none, `max_idle_fraction` then limits nothing and `stats["idle_steps"]` stays 0.  `stats["row_forwards"]` counts the
    rows the calls' forwards ran, with or without it.  EchoHipError on an fp8 model, at construction."""

    def __init__(self, model, fish_ae, pca_state, voices=None, max_batch: int = 24, mix_block_sizes: bool = False,
                 max_pad_fraction: Optional[float] = None, batch_decode: bool = False, mix_steps: bool = False,
                 max_idle_fraction: Optional[float] = None, compact_rows: bool = False):
        from .handler import VoiceCache
        from ._lib import EchoHipError
        if compact_rows and getattr(model, "fp8", False):
            raise EchoHipError("compact_rows: not supported by the fp8 engine (dit_fp8): its e4m3 attention output has no row-map form; "
                               "use the bf16 engine")
        self.compact_rows = bool(compact_rows)
        if mix_steps and not mix_block_sizes:
            raise ValueError("mix_steps=True requires mix_block_sizes=True: a call that mixes step counts is planned by plan_stream_step_mixed")
        self.mix_steps, self.max_idle_fraction = bool(mix_steps), max_idle_fraction
        self.model, self.fish_ae, self.pca_state = model, fish_ae, pca_state
        self.batch_decode = bool(batch_decode)
        self.max_batch = max(1, min(int(max_batch), MAX_ITEMS))
        self.mix_block_sizes, self.max_pad_fraction = bool(mix_block_sizes), max_pad_fraction
        self._cache = voices if isinstance(voices, VoiceCache) else VoiceCache()
        self._registry = {} if isinstance(voices, VoiceCache) or voices is None else dict(voices)
        self._streams: Dict[int, StreamState] = {}
        self._next_id = 0
        self._tick = 0
        # ms_*: filled when `timing` is set (adds synchronisation); tokens / pad_tokens: token rows the calls carried / of them padding
        # steps / idle_steps: (stream, iteration) pairs the calls ran / of them past the stream's own last step
        self.stats = {"calls": 0, "rows": 0, "ms_encode": 0.0, "ms_sample": 0.0, "tokens": 0, "pad_tokens": 0, "steps": 0, "idle_steps": 0,
                      "row_forwards": 0}
        self.timing = False

    # ------------------------------------------------------------------ voices
    def _voice(self, v):
        from .inference import get_speaker_latent_and_mask
        from .model import VoiceHandle
        if isinstance(v, VoiceHandle):
            if v.batch != 1:
                raise ValueError("speaker_voice: a captured voice must have batch size 1")
            return v
        m = self.model
        key = _NO_VOICE if v is None else v
        if self._cache.latent(key) is None:
            if v is None:
                lz = m.config.latent_size
                lat, mask = torch.zeros((1, 4, lz), device=m.device, dtype=m.dtype), torch.zeros((1, 4), device=m.device, dtype=torch.bool)
            else:
                src = self._registry.get(v)
                if src is None:
                    raise ValueError(f"speaker_voice '{v}' not found")
                lat, mask = src if isinstance(src, (tuple, list)) else get_speaker_latent_and_mask(self.fish_ae, self.pca_state, src.to(m.device))
            self._cache.put_latent(key, lat.to(m.device, m.dtype), mask)
        return self._cache.speaker_kv(m, key)

    # ------------------------------------------------------------------ streams
    def open(self, text_input_ids, text_mask, item_params: dict, block_sizes: Sequence[int], rng_seed: int, speaker_voice=None,
             continuation_latent: Optional[torch.Tensor] = None, x_inits: Optional[List[torch.Tensor]] = None) -> int:
        """One utterance: text_input_ids / text_mask (1, Tt) or (Tt,); `item_params` = the reference's per-request sampler keys
        (STREAM_ITEM_KEYS); `x_inits` (one (1, block, latent) or (block, latent) tensor per block) replaces the RNG draw, which is otherwise
        the draw `sample_blockwise_stream` makes for a batch-1 request with `rng_seed`.  Returns the stream's id."""
        m = self.model
        item = dict(item_params)
        cont_len = 0 if continuation_latent is None else int(continuation_latent.shape[-2])
        check_stream_request(item, block_sizes, cont_len, int(getattr(m, "MAX_POS", 4096)))
        if not m.has_latent_encoder:
            raise RuntimeError("this checkpoint was loaded without the blockwise modules")
        ids = text_input_ids.reshape(1, -1).to(m.device, torch.int32)
        tmask = torch.ones_like(ids, dtype=torch.bool) if text_mask is None else text_mask.reshape(1, -1).to(m.device, torch.bool)
        if x_inits is not None and len(x_inits) != len(block_sizes):
            raise ValueError("x_inits: one noise tensor per block expected")
        lz = m.config.latent_size
        prefix = torch.zeros((cont_len + sum(int(b) for b in block_sizes), lz), device=m.device, dtype=torch.float32)
        if cont_len:
            prefix[:cont_len] = continuation_latent.reshape(cont_len, lz).to(m.device, torch.float32)
        sid = self._next_id
        self._next_id += 1
        st = StreamState(id=sid, arrival=sid, block_sizes=tuple(int(b) for b in block_sizes), num_steps=int(item["num_steps"]),
                         waiting_since=self._tick, item=item, ids=ids, tmask=tmask, voice=self._voice(speaker_voice), prefix=prefix,
                         start=cont_len, x_inits=None if x_inits is None else list(x_inits),
                         rng=torch.Generator(device=m.device).manual_seed(int(rng_seed)))
        self._streams[sid] = st
        return sid

    def close(self, sid: int) -> None:
        self._streams.pop(sid, None)

    @property
    def open_ids(self) -> List[int]:
        return [s.id for s in self._streams.values() if not s.finished]

    def latents(self, sid: int) -> torch.Tensor:
        """(1, latents so far, latent_size) of an open stream: continuation + generated blocks."""
        s = self._streams[sid]
        return s.prefix[:s.start].unsqueeze(0)

    def _noise(self, s: StreamState) -> torch.Tensor:
        bs, lz = s.block_sizes[s.next_block], self.model.config.latent_size
        if s.x_inits is not None:
            return s.x_inits[s.next_block].reshape(1, bs, lz).to(self.model.device, torch.float32)
        return torch.randn((1, bs, lz), device=self.model.device, dtype=torch.float32, generator=s.rng)

    def step(self) -> List[Tuple[int, int, torch.Tensor]]:
        """One sampler call.  Returns [(id, start_pos, block_latents (1, block_size, latent))] of the streams it carried ([] when none is
        open).  A stream closes itself after its last block."""
        out = self._step()
        self._reap()
        return out

    @torch.inference_mode()
    def _step(self) -> List[Tuple[int, int, torch.Tensor]]:
        from .inference import _multiply_kv_cache_items, build_sampler_items, check_sampler_items, check_sampler_items_steps, run_euler_items
        if self.mix_block_sizes:
            picked = plan_stream_step_mixed(list(self._streams.values()), self.max_batch, self.max_pad_fraction, mix_steps=self.mix_steps, compact=self.compact_rows,
                                            max_idle_fraction=self.max_idle_fraction)
        else:
            picked = plan_stream_step(list(self._streams.values()), self.max_batch)
        if not picked:
            return []
        m = self.model
        rows = [self._streams[i] for i in picked]
        if self.mix_steps:       # equal step counts next to each other (one modulation segment per run of rows), longest first, stable
            rows.sort(key=lambda s: -int(s.num_steps))
        B, ps = len(rows), m.config.speaker_patch_size
        items = [dict(s.item) for s in rows]
        counts = [int(s.num_steps) for s in rows]
        mixed_steps = len(set(counts)) > 1           # only with mix_steps
        if mixed_steps:
            check_sampler_items_steps(items, B, B, need_seed=False)
        else:
            check_sampler_items(items, B, B, need_seed=False)
        arr, temb, _keep = build_sampler_items(m, items)
        if self.timing:
            torch.cuda.synchronize(m.device)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
        # texts: padded to the call's longest, each behind its own key mask
        Tt = max(int(s.ids.shape[1]) for s in rows)
        ids = torch.zeros((B, Tt), device=m.device, dtype=torch.int32)
        tmask = torch.zeros((B, Tt), device=m.device, dtype=torch.bool)
        for b, s in enumerate(rows):
            ids[b, :s.ids.shape[1]] = s.ids[0]
            tmask[b, :s.tmask.shape[1]] = s.tmask[0]
        m.get_kv_cache_text(ids, tmask)
        kv_spk = m.bind_voices([s.voice for s in rows])
        if any(it["speaker_kv_scale"] is not None for it in items):
            _multiply_kv_cache_items(kv_spk, [1.0 if it["speaker_kv_scale"] is None else it["speaker_kv_scale"] for it in items],
                                     [it["speaker_kv_max_layers"] for it in items])
        # prefixes: one encode up to the longest item's prefix; an item's rows beyond its own prefix are zeros (finite, masked by count)
        starts = [int(s.start) for s in rows]
        n_lat = (max(starts) + ps - 1) // ps * ps
        P = max(n_lat, ps)
        stacked = torch.zeros((B, P, m.config.latent_size), device=m.device, dtype=torch.float32)
        for b, s in enumerate(rows):
            stacked[b, :s.start] = s.prefix[:s.start]
        m.get_kv_cache_latent(stacked, n_latents=n_lat)
        sizes = [int(s.block_sizes[s.next_block]) for s in rows]
        mixed = len(set(sizes)) > 1                  # only with mix_block_sizes: every stream's own noise in a zero (B, S_call, latent) tensor
        if mixed:
            x0 = torch.zeros((B, max(sizes), m.config.latent_size), device=m.device, dtype=torch.float32)
            for b, s in enumerate(rows):
                x0[b, :sizes[b]] = self._noise(s)[0]
        else:
            x0 = torch.cat([self._noise(s) for s in rows], 0)
        if self.timing:
            ev[1].record()
        if mixed_steps:
            x = run_euler_items(m, x0, arr, max(counts), None, start_pos=starts, use_latent=True, lengths=sizes if mixed else None,
                                item_steps=counts, compact_rows=self.compact_rows)
        elif mixed:
            x = run_euler_items(m, x0, arr, rows[0].num_steps, temb, start_pos=starts, use_latent=True, lengths=sizes, compact_rows=self.compact_rows)
        else:
            x = run_euler_items(m, x0, arr, rows[0].num_steps, temb, start_pos=starts, use_latent=True, compact_rows=self.compact_rows)
        self.stats["row_forwards"] += m.last_row_forwards()
        if self.timing:
            ev[2].record()
            torch.cuda.synchronize(m.device)
            self.stats["ms_encode"] += ev[0].elapsed_time(ev[1])
            self.stats["ms_sample"] += ev[1].elapsed_time(ev[2])
        self.stats["calls"] += 1
        self.stats["rows"] += B
        self.stats["tokens"] += B * max(sizes)
        self.stats["pad_tokens"] += B * max(sizes) - sum(sizes)
        self.stats["steps"] += B * max(counts)
        self.stats["idle_steps"] += 0 if self.compact_rows else B * max(counts) - sum(counts)
        self._tick += 1
        out = []
        for b, s in enumerate(rows):
            bs = s.block_sizes[s.next_block]
            s.prefix[s.start:s.start + bs] = x[b, :bs]
            out.append((s.id, s.start, x[b:b + 1, :bs]))
            s.start += bs
            s.next_block += 1
            s.waiting_since = self._tick
        return out

    def _reap(self) -> None:
        for sid in [s.id for s in self._streams.values() if s.finished]:
            self._streams.pop(sid)

    @torch.inference_mode()
    def step_audio(self) -> List[Tuple[int, torch.Tensor]]:
        """`step()`, then each new block through its stream's own `DACStream` (batch 1): [(id, waveform chunk (1, 1, block_size * hop))].
        The concatenated chunks of a stream equal `ae_decode` of its final latent."""
        from .autoencoder import DACStream
        if self.batch_decode:
            return self._step_audio_batched()
        out = []
        for sid, start, block in self._step():
            s = self._streams[sid]
            if s.dec is None:
                s.dec = DACStream(self.fish_ae, self.pca_state)
                if start > 0:                    # a continuation's audio exists already: only its decoder context is needed
                    s.dec.push(s.prefix[:start])
            out.append((sid, s.dec.push(block[0])))
        self._reap()
        return out


    def _step_audio_batched(self) -> List[Tuple[int, torch.Tensor]]:
        """`step_audio` with one engine call for the step's decodes: the continuation prefixes of streams that decode for the first time go
        through one `push_many` (their audio exists already: only the decoder context is needed), the new blocks through a second one."""
        from .autoencoder import DACStream
        got = self._step()
        if not got:
            self._reap()
            return []
        rows = [self._streams[sid] for sid, _, _ in got]
        fresh = []
        for s, (_, start, _) in zip(rows, got):
            if s.dec is None:
                s.dec = DACStream(self.fish_ae, self.pca_state)
                if start > 0:
                    fresh.append((s.dec, s.prefix[:start]))
        if fresh:
            DACStream.push_many([d for d, _ in fresh], [p for _, p in fresh])
        chunks = DACStream.push_many([s.dec for s in rows], [block[0] for _, _, block in got])
        self._reap()
        return [(sid, chunk) for (sid, _, _), chunk in zip(got, chunks)]


def stream_audio_many(model, fish_ae, pca_state, requests: Sequence[dict], voices=None, max_batch: int = 24, mix_block_sizes: bool = False,
                      max_pad_fraction: Optional[float] = None, batch_decode: bool = False, mix_steps: bool = False,
                      max_idle_fraction: Optional[float] = None, compact_rows: bool = False) -> Iterator[Tuple[int, torch.Tensor]]:
    """Generator over a list of requests (dicts with the keyword arguments of `StreamBatcher.open`): opens them all and yields
    `(request index, waveform chunk)` block by block until every stream is done.  `mix_block_sizes` / `max_pad_fraction` / `batch_decode` /
    `mix_steps` / `max_idle_fraction` / `compact_rows`: `StreamBatcher`."""
    sb = StreamBatcher(model, fish_ae, pca_state, voices=voices, max_batch=max_batch, mix_block_sizes=mix_block_sizes,
                       max_pad_fraction=max_pad_fraction, batch_decode=batch_decode, mix_steps=mix_steps, max_idle_fraction=max_idle_fraction,
                       compact_rows=compact_rows)
    index = {sb.open(**dict(r)): i for i, r in enumerate(requests)}
    while sb.open_ids:
        for sid, chunk in sb.step_audio():
            yield index[sid], chunk
