"""Batch pipeline for serving loops: several decode chains in flight, the acoustic stages behind them.

The reference synthesises one request after the other (infer_v2.py:732, serve_tars.py's single worker).  On an MI355X the two
halves of a batch behave differently: the autoregressive decode (`IndexTTS2.gpt_stage`) is a chain of ~125 small dependent
launches per token that leaves most CUs idle at any instant, s2mel + vocoder (`IndexTTS2.acoustic_stage`) are MFMA- / HBM-bound
and fill the chip.  `BatchPipeline` keeps `decode_lanes` decode chains running at once -- each on its own HIP stream, driven by its
own host thread (the C call releases the GIL), with its own KV-cache workspace -- and runs the acoustic stages on
`acoustic_workers` further streams.

`acoustic_coalesce` > 1 lets a free acoustic worker take that many decoded requests (same prompt, or any prompts with
`acoustic_mix_prompts=True`; explicit CFM noise, or a `noise_seed`) as ONE s2mel + vocoder batch; `coalesce` > 1 is dynamic batching of the decode: a
lane that becomes free takes up to `coalesce` waiting requests of the same
prompt and text width and decodes them as ONE batch (a decode step streams the 965 MB of GPT weights once whatever the number of rows, so two
16-utterance requests decoded together cost little more than one), then hands every request's rows to its own acoustic job.

Every request is computed exactly as `synthesize_batch` computes it: the kernels treat the rows of a batch independently (same
arithmetic and summation order per row whatever the batch size: tests/test_serving_gpu.py, and bench.py compares every retired
batch with the sequential call bit for bit), so only the interleaving on the device changes.  Two launches pick their KERNEL by
row count, though, and a merge must not move a request across either threshold (`merge_keeps_kernels`, enforced in `_take`):
the GEMM-shaped passes run split-bf16 from 256 rows up (a request of a few dozen prefill rows would change kernels when merged --
what made `test_batch_pipeline_equals_sequential[2-3-2]` differ from the sequential call at the 1e-4 level in round 3, on toy
requests of 38-76 rows; any real utterance is hundreds of rows on its own), and the decode step runs on the plane GEMV from
`idxtts_set_decode_plane_rows()` rows on (default 17) -- so 16-utterance requests merge only where the plane GEMV also decodes
them alone (`_lib.set_decode_plane_rows(5)`, once per process), or where the merged batch stays below the threshold.

Measured at configs[2] (profiles/README.md "Round 3"): decode chains and acoustic stages SHARING the device give the same
throughput as strict turns (3 decodes together, then their 3 acoustic stages: 163 vs 165 audio-s/s) -- a decode launch that needs
240-320 one-round workgroups waits for the 256x256-tile GEMMs of an acoustic stage to give CUs back anyway (their workgroups own
a CU's whole register file) -- so there is one schedule: sharing.

    _lib.set_decode_geometry(True)           # once per process, before generating: decode GEMVs as 512-thread workgroups, which find room
                                             # beside the acoustic stage's kernels (+1.5 % here, 7 % slower for a decode alone)
    pipe = BatchPipeline(tts, decode_lanes=3)
    futs = [pipe.submit(text_k, cond, max_mel_tokens=..., noise_seed=seed_k) for text_k in batches]      # or noise=noise_k
    wavs = [f.result() for f in futs]        # lists of [1, n] waveforms, as synthesize_batch returns them
    pipe.close()
"""
from __future__ import annotations

import collections
import concurrent.futures
import contextlib
import operator
import threading
import time
from typing import Optional

import torch


def merge_keeps_kernels(rows_each, prefix_len: int, split_bf16_gemm: bool, compact_weights: bool, plane_rows: int,
                        batch_invariant: bool = False) -> bool:
    """May requests of `rows_each` utterances (same text width; `prefix_len` = conditioning + text rows of one utterance's prompt) be
    decoded as ONE batch and still equal their own sequential calls bit for bit?  Rows are independent inside every kernel; what a merge
    can change is WHICH kernel runs:
      * GEMM-shaped passes (prefill, latent pass): exact fp32 below 256 rows, split-bf16 from 256 rows on (csrc/gemm.hip dispatch) --
        every request must be on the split-bf16 side by itself (its prefill alone has >= 256 rows), unless the exact mode is selected;
      * the decode step with compact weight streams: fp32-MFMA GEMV below `plane_rows` rows, plane GEMV from there on
        (idxtts_set_decode_plane_rows) -- all requests and the merged batch must fall on the same side.
    batch_invariant (UnifiedVoice.set_batch_invariant): every launch that feeds the choice of a code follows the request alone, so
    any merge keeps every request's codes."""
    rows_each = [int(r) for r in rows_each]
    if len(rows_each) <= 1 or batch_invariant:
        return True
    if split_bf16_gemm and any(r * prefix_len < 256 for r in rows_each):
        return False
    if compact_weights:
        total = sum(rows_each)
        if not (total < plane_rows or min(rows_each) >= plane_rows):
            return False
    return True


def _draw_seeds(n: int, seed=None, generator=None) -> list:
    """The one seed rule: n seeds, each torch.randint(0, 2**62, (1,), generator=g), drawn one after the other with g =
    torch.Generator().manual_seed(seed) when `seed` is given, else `generator`, else (None) torch's global RNG."""
    g = torch.Generator().manual_seed(int(seed)) if seed is not None else generator
    return [int(torch.randint(0, 2 ** 62, (1,), generator=g).item()) for _ in range(n)]


def utterance_noise_seeds(noise_seed, n: int):
    """The per-utterance CFM noise seeds of a request of `n` utterances (IndexTTS2.acoustic_stage's `noise_seeds`).  None: None (the
    noise is given, or drawn from torch's generator).  An int: n seeds drawn as utterance_samplers draws its seeds,
    torch.randint(0, 2**62, (1,), generator=torch.Generator().manual_seed(noise_seed)) in utterance order.  A sequence of n ints
    (0 <= s < 2**64): taken as given.  Raises ValueError on anything else."""
    if noise_seed is None:
        return None
    if isinstance(noise_seed, int) and not isinstance(noise_seed, bool):
        if not 0 <= noise_seed < 2 ** 64:
            raise ValueError("noise_seed must be in 0 <= seed < 2**64")
        return _draw_seeds(n, seed=noise_seed)
    try:
        seeds = [operator.index(v) for v in noise_seed]
    except TypeError:
        raise ValueError("noise_seed must be None, an int or a sequence of one int per utterance") from None
    if len(seeds) != n:
        raise ValueError(f"{len(seeds)} noise seeds for {n} utterances")
    if any(not 0 <= v < 2 ** 64 for v in seeds):
        raise ValueError("noise seeds must be in 0 <= seed < 2**64")
    return seeds


def _noise_kind(r) -> int:
    """How a request's CFM noise is fixed: 1 = explicit tensor, 2 = seeds, 0 = neither (drawn when its acoustic stage runs, so it is
    never merged).  Only requests of one non-zero kind share an acoustic batch."""
    return 1 if r.noise is not None else 2 if r.noise_seeds is not None else 0


def _noise_of(r):
    return r.noise if r.noise is not None else r.noise_seeds


def acoustic_settings(diffusion_steps, cfg_rate, rows: int):
    """A request's CFM solver settings as submitted -> (steps, rates): each None (not given: the pipeline's defaults) or a list of one
    value per row.  One value applies to every row; a sequence has one entry per row -- for a request with takes per row i * takes + j,
    utterance_noise_seeds' rule.  ValueError: a wrong length, steps < 1, a negative or non-finite rate."""
    from .s2mel import per_row_values
    return (None if diffusion_steps is None else per_row_values(diffusion_steps, rows, "diffusion_steps")[0],
            None if cfg_rate is None else per_row_values(cfg_rate, rows, "cfg_rate")[0])


def merge_acoustic_states(items, defaults=None):
    """Several requests' `gpt_stage` states as ONE acoustic batch.  items: (cond, state, noise) per request, `cond` being what the
    request was submitted with (one PromptConditioning, or one per row).  Rows are independent in s2mel and the vocoder (ragged
    lengths: every row is padded at its own end), so stacking them only changes how the launches fill the chip.  Requests of ONE
    prompt keep the single-prompt path (state["cond"] = that prompt); otherwise state["cond"] is the list of every row's prompt
    (IndexTTS2.acoustic_stage then runs S2Mel.cfm_rows), rows submitted with the same object sharing one device copy.  Each request's
    noise keeps its rows' frames from column 0 and is zero-padded on the right.  Returns (state, noise).  Seeded requests pass
    their list of per-row seeds in place of the noise tensor (every item, or none): the second value is then the concatenated
    list, in row order.
    Per-row solver settings: a state may carry "diffusion_steps" / "cfg_rate", one value per row (a request submitted with them).  If
    any does, the merged state carries the key with a value for every row, the rows of a state without it taking defaults =
    (diffusion_steps, cfg_rate), the pipeline's; if none does, the merged state has neither key."""
    sts = [st for _, st, _ in items]
    n = max(st["codes"].shape[1] for st in sts)
    codes = torch.cat([torch.nn.functional.pad(st["codes"], (0, n - st["codes"].shape[1])) for st in sts])
    latent = torch.cat([torch.nn.functional.pad(st["latent"], (0, 0, 0, n - st["latent"].shape[1])) for st in sts])
    if all(isinstance(z, (list, tuple)) for _, _, z in items):
        noise = [int(s) for _, _, z in items for s in z]
    else:
        T = max(z.shape[-1] for _, _, z in items)
        noise = torch.cat([torch.nn.functional.pad(z, (0, T - z.shape[-1])) for _, _, z in items])
    keys, first = [], {}
    for cond, st, _ in items:
        dc = st["cond"]
        for b in range(st["B"]):
            k = id(cond[b]) if isinstance(cond, (list, tuple)) else id(cond)
            first.setdefault(k, dc[b] if isinstance(dc, list) else dc)
            keys.append(k)
    rows = [first[k] for k in keys]
    cond = sts[0]["cond"] if all(k == keys[0] for k in keys) else rows
    st = {"cond": cond, "B": sum(st["B"] for st in sts), "codes": codes, "code_lens": [c for st in sts for c in st["code_lens"]],
          "code_lens_t": torch.cat([st["code_lens_t"] for st in sts]), "latent": latent, "times": dict(sts[0]["times"])}
    for key, dflt in zip(("diffusion_steps", "cfg_rate"), defaults or (None, None)):
        if any(key in s for s in sts):
            if dflt is None and not all(key in s for s in sts):
                raise ValueError(f"merging requests with and without {key} needs the pipeline's default")
            st[key] = [v for s in sts for v in (s[key] if key in s else [dflt] * s["B"])]
    return st, noise


def rank_request(codes, logprobs, takes: int, stop_token: int, length_penalty: float = 1.0) -> list:
    """The takes of every utterance of a request, ranked.  codes / logprobs: one 1-D row per take (row i * takes + j: take j of
    utterance i), each as long as the take (the stop token included).  Returns ranking[i]: all `takes` takes of utterance i, best first,
    as (take_index, score, stopped, n_codes) -- score = gpt.sequence_scores (the sum of the codes' log-probabilities over
    n_codes ** length_penalty, float64), stopped = the last code is the stop token, order = gpt.rank_takes (stopped first, higher score,
    lower index): a take that ran into its cap ranks below every take that stopped."""
    from .gpt import rank_takes, sequence_scores
    takes = int(takes)
    lens = [int(c.shape[0]) for c in codes]
    if len(codes) != len(logprobs) or len(codes) % takes or any(int(lp.shape[0]) != n for lp, n in zip(logprobs, lens)):
        raise ValueError("one row of log-probabilities per row of codes, of the same length, `takes` rows per utterance")
    scores = sequence_scores(logprobs, lens, length_penalty)
    stopped = [int(c[-1]) == int(stop_token) for c in codes]
    out = []
    for a in range(0, len(codes), takes):
        order = rank_takes(scores[a:a + takes], stopped[a:a + takes])
        out.append([(t, float(scores[a + t]), stopped[a + t], lens[a + t]) for t in order])
    return out


def _keep_best(r, ranking, keep: int) -> list:
    """Cuts a request with r.takes takes per utterance down to the best `keep` of each, best first: its text,
    per-row prompts, CFM noise rows, noise seeds and solver settings follow the kept takes (take j of utterance i keeps entry i * takes + j), and r.takes
    becomes `keep`.  Returns the kept rows' indices."""
    rows = [i * r.takes + rk[q][0] for i, rk in enumerate(ranking) for q in range(keep)]
    r.text = r.text[rows]
    if isinstance(r.cond, (list, tuple)):
        r.cond = [r.cond[q] for q in rows]
    if r.noise is not None:
        r.noise = r.noise[rows]
    if r.noise_seeds is not None:
        r.noise_seeds = [r.noise_seeds[q] for q in rows]
    if r.diffusion_steps is not None:
        r.diffusion_steps = [r.diffusion_steps[q] for q in rows]
    if r.cfg_rate is not None:
        r.cfg_rate = [r.cfg_rate[q] for q in rows]
    r.takes = keep
    return rows


def _check_keep(keep, takes: int, scored: bool, beam: bool):
    """submit(keep=): None, or 1 <= keep <= takes on a pipeline that scores sampled takes."""
    if keep is None:
        return None
    if beam:
        raise ValueError("keep on a beam pipeline: `takes` already returns the scorer's n best hypotheses, best first")
    if not scored:
        raise ValueError("keep needs the takes' scores: build the pipeline with scores=True")
    keep = int(keep)
    if not 1 <= keep <= takes:
        raise ValueError("keep must be in 1 .. takes")
    return keep


def _set_exception(fut, e: BaseException) -> None:
    """A failure handed to a request that has no outcome yet.  A cancelled request has one: it is left alone, also when the caller's
    cancel() lands between the check and the call."""
    try:
        if not fut.done():
            fut.set_exception(e)
    except concurrent.futures.InvalidStateError:
        pass


_NOTIFY = threading.Lock()


def _cancelled(owner) -> bool:
    """Has the request's Future (owner.done) been cancelled?  Whoever sees it first tells the Future's waiters: concurrent.futures.wait
    and as_completed count a cancelled Future only once set_running_or_notify_cancel has been called on it, and a second call is an
    error, hence the flag."""
    if not owner.done.cancelled():
        return False
    with _NOTIFY:
        if not owner.notified:
            owner.notified = True
            owner.done.set_running_or_notify_cancel()
    return True


def _start(owner) -> bool:
    """The point of no return: marks the request running, after which cancel() on its Future returns False.  False: the request was
    cancelled first (its waiters are told), or it already has an outcome."""
    fut = owner.done
    with _NOTIFY:
        if owner.notified or (fut.done() and not fut.cancelled()):
            return False
        if fut.set_running_or_notify_cancel():
            return True
        owner.notified = True
        return False


def _expand_cond(cond, n: int):
    """The conditioning of a request with n takes per utterance, one entry per take (row i * n + j: utterance i): a list of prompts is
    repeated entry by entry; one prompt for every row (leading dimension 1) serves as it is."""
    if isinstance(cond, (list, tuple)):
        return [c for c in cond for _ in range(n)]
    if int(cond.spk_cond_latent.shape[0]) == 1 and int(cond.emo_vec.shape[0]) == 1:
        return cond
    raise ValueError("takes > 1 needs one prompt for the whole request, or a list of one prompt per utterance")


class _Request:
    """One submitted batch of utterances, one row per take (_new_request).  A BatchPipeline adds what its one-shot decode needs and
    leaves behind (repetition_penalty, base, state); a ContinuousPipeline, whose rows decode independently in whatever slots are free,
    adds the decode's progress (codes .. prefix_lps)."""
    __slots__ = ("text", "cond", "max_mel_tokens", "noise", "noise_seeds", "sampling", "ready", "caller", "done", "notified", "takes", "keep",
                 "repetition_penalty", "base", "state", "diffusion_steps", "cfg_rate",
                 "codes", "left", "failed", "seq", "deadline", "priority", "stamp", "nbest", "lps", "prefix", "prefix_lps")

    def compatible(self, other: "_Request") -> bool:
        # same prompt and settings, greedy (sampling draws are per call) and the SAME text width: a wider neighbour would left-pad this
        # request's prompts further, which moves the key-tile boundaries of the prefill attention (a different fp32 summation order)
        return (self.cond is other.cond and self.max_mel_tokens == other.max_mel_tokens and self.repetition_penalty == other.repetition_penalty
                and self.sampling is None and other.sampling is None and int(self.text.shape[1]) == int(other.text.shape[1]))


# One utterance's rows in a ContinuousPipeline admission: its prompt, the (request, row) of every take admitted with it and, per take,
# the cap and the sampler (None on a greedy pipeline; a beam pipeline: the group's one beam entry), the codes it continues from
_Part = collections.namedtuple("_Part", "prompt owners caps samplers prefix prefix_lps")


class _Pipeline:
    """What the two pipelines do the same way: build a request, give every worker thread its stream, run the acoustic jobs on
    `acoustic_workers` threads, hand the waveforms back, release the streams.  Which decoded requests make the next acoustic job
    (_take_acoustic), where a request's gpt_stage state comes from (_acoustic_state), what retiring a job does (_retire) and what its
    trace entry holds (_acoustic_entry) are each pipeline's own."""

    def __init__(self, tts, acoustic_workers: int, lock, cuda: bool):
        self.tts = tts
        self.device = torch.device(tts.device)
        self._cuda = cuda                      # off-GPU (a ContinuousPipeline of stand-in sessions) there are no streams and no events
        self._lock = lock                      # the pipeline's own lock, taken here where the list of streams grows
        self._pri = {"decode": 0, "acoustic": 0}      # stream priority by kind of worker (0: the default)
        self._tls = threading.local()          # one stream per worker THREAD: two jobs never share a stream (= a workspace)
        self._streams = []                     # every worker thread's stream (handed back to the library in close())
        self._turn = contextlib.nullcontext()  # held around a job's GPU work
        self._aq = collections.deque()         # decoded requests waiting for an acoustic worker
        self._acoustic = concurrent.futures.ThreadPoolExecutor(max_workers=acoustic_workers, thread_name_prefix="idxtts-acoustic")
        self.trace = None                      # set to a list to record the host times (time.perf_counter) of the jobs

    def _new_request(self, text_tokens, cond, max_mel_tokens, noise, noise_seed, takes: int, keep, samplers=None, diffusion_steps=None,
                     cfg_rate=None) -> _Request:
        """A request as submitted: its Future (r.done), the text and conditioning with every utterance repeated `takes` times (row
        i * takes + j: take j of utterance i), the rows' CFM noise or noise seeds, then -- drawn after the noise seeds -- r.sampling =
        samplers(rows), what the pipeline fixes per row, and the caller's stream with the event recorded on it that the workers wait for
        (both None off-GPU).  A bad noise / noise_seed, a conditioning that cannot be repeated and a ValueError of `samplers` fail the
        Future only: the request then comes back done and is not to be queued."""
        r = _Request()
        r.done, r.notified, r.takes, r.keep = concurrent.futures.Future(), False, takes, keep
        r.text, r.cond, r.max_mel_tokens = torch.as_tensor(text_tokens), cond, max_mel_tokens
        try:
            if takes > 1:
                r.text, r.cond = r.text.repeat_interleave(takes, 0), _expand_cond(cond, takes)
            rows = int(r.text.shape[0])
            if noise is not None and noise_seed is not None:
                raise ValueError("pass `noise` or `noise_seed`, not both")
            r.noise, r.noise_seeds = noise, utterance_noise_seeds(noise_seed, rows)
            r.diffusion_steps, r.cfg_rate = acoustic_settings(diffusion_steps, cfg_rate, rows)
            r.sampling = samplers(rows) if samplers is not None else None
        except ValueError as e:
            r.done.set_exception(e)
            return r
        r.caller = torch.cuda.current_stream(self.device) if self._cuda else None
        r.ready = torch.cuda.Event() if self._cuda else None
        if self._cuda:
            r.ready.record(r.caller)
        return r

    def _stream(self, kind: str):
        """The calling worker thread's stream, made at its first job; None off-GPU."""
        s = getattr(self._tls, "stream", None)
        if s is None and self._cuda:
            s = self._tls.stream = torch.cuda.Stream(device=self.device, priority=self._pri[kind])
            with self._lock:
                self._streams.append(s)
        return s

    def _on(self, s):
        return torch.cuda.stream(s) if s is not None else contextlib.nullcontext()

    def _wait_ready(self, r: _Request) -> None:
        """The current stream waits for what the caller's stream held when the request was submitted."""
        if r.ready is not None:
            torch.cuda.current_stream(self.device).wait_event(r.ready)

    @staticmethod
    def _fail(r: _Request, e: BaseException) -> None:
        r.failed = True
        _set_exception(r.done, e)

    def _retire(self, group) -> None:
        """An acoustic job's requests have their outcome."""

    def _acoustic_entry(self, t0: float, t1: float, rows: int, group) -> tuple:
        """What `trace` records of an acoustic job: (kind, start, end, rows), as of every job."""
        return ("acoustic", t0, t1, rows)

    def _acoustic_drain(self):
        """One acoustic job: the group's states (merge_acoustic_states; one request: its own) through s2mel and the vocoder as one
        batch, and every request its own rows.  A failure fails every request of the job and nothing else."""
        group = self._take_acoustic()
        if not group:
            return
        try:
            if self._cuda:
                torch.cuda.set_device(self.device)
            t0 = time.perf_counter()
            sa = self._stream("acoustic")
            with self._turn, self._on(sa):
                states = [self._with_settings(r, self._acoustic_state(r)) for r in group]
                if len(group) == 1:
                    st, noise = states[0], _noise_of(group[0])
                else:
                    st, noise = merge_acoustic_states([(r.cond, s, _noise_of(r)) for r, s in zip(group, states)],
                                                      (getattr(self.tts, "_diffusion_steps", None), getattr(self.tts, "_cfg_rate", None)))
                kw = {"noise_seeds": noise} if isinstance(noise, list) else {"noise": noise}      # a tensor, None or a seed list
                wavs = self.tts.acoustic_stage(st, **kw)
                if sa is not None:
                    sa.synchronize()            # the states' tensors may be released once this returns
            rows = [int(r.text.shape[0]) for r in group]
            if self.trace is not None:
                self.trace.append(self._acoustic_entry(t0, time.perf_counter(), sum(rows), group))
            a = 0
            for r, n in zip(group, rows):
                self._deliver(r, wavs[a:a + n])
                a += n
        except BaseException as e:              # noqa: BLE001 -- handed to the callers through their futures
            for r in group:
                self._fail(r, e)
        finally:
            self._retire(group)

    @staticmethod
    def _with_settings(r: _Request, st: dict) -> dict:
        """The request's gpt_stage state with its per-row solver settings, where it was submitted with any (acoustic_stage reads them
        from the state); otherwise the state as it is."""
        if r.diffusion_steps is None and r.cfg_rate is None:
            return st
        st = dict(st)
        if r.diffusion_steps is not None:
            st["diffusion_steps"] = list(r.diffusion_steps)
        if r.cfg_rate is not None:
            st["cfg_rate"] = list(r.cfg_rate)
        return st

    @staticmethod
    def _deliver(r: _Request, wavs: list) -> None:
        """A request's waveforms to its Future: the flat list, or result[i][j] for a request with takes (or keep)."""
        if r.caller is not None:
            for w in wavs:                      # allocated on the worker's stream, consumed on the caller's
                w.record_stream(r.caller)
        r.done.set_result(wavs if r.takes == 1 and r.keep is None else [wavs[i:i + r.takes] for i in range(0, len(wavs), r.takes)])

    def _close_acoustic(self):
        """The end of close(), once nothing decodes any more: the acoustic jobs drain, then the library's per-stream scratch goes
        with the worker threads' streams."""
        self._acoustic.shutdown(wait=True)
        if self._cuda:
            from . import _lib
            with torch.cuda.device(self.device):
                for s in self._streams:
                    s.synchronize()
                    _lib.release_stream(s)
        self._streams = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class BatchPipeline(_Pipeline):
    def __init__(self, tts, decode_lanes: int = 3, acoustic_workers: int = 1, coalesce: int = 1, lane_priority: str = "high",
                 acoustic_coalesce: int = 1, exclusive: bool = False, acoustic_mix_prompts: bool = False):
        """acoustic_mix_prompts: let `acoustic_coalesce` merge decoded requests of DIFFERENT prompts into one acoustic batch (a
        mixed-prompt CFM, S2Mel.cfm_rows); default: only requests of one prompt object are merged."""
        if decode_lanes < 1 or acoustic_workers < 1 or coalesce < 1 or acoustic_coalesce < 1:
            raise ValueError("decode_lanes, acoustic_workers, coalesce and acoustic_coalesce must be >= 1")
        self._qlock = threading.Lock()
        super().__init__(tts, acoustic_workers, self._qlock, cuda=True)      # (every stage of this pipeline is a GPU stage)
        self.decode_lanes = decode_lanes
        self.acoustic_workers = acoustic_workers
        self.coalesce = coalesce
        self.acoustic_coalesce = acoustic_coalesce
        self.acoustic_mix_prompts = bool(acoustic_mix_prompts)
        lo_pri, hi_pri = torch.cuda.Stream.priority_range() if hasattr(torch.cuda.Stream, "priority_range") else (0, -1)
        self._pri = {"decode": hi_pri if lane_priority == "high" else lo_pri, "acoustic": lo_pri}
        self._lanes = concurrent.futures.ThreadPoolExecutor(max_workers=decode_lanes, thread_name_prefix="idxtts-decode")
        self._queue = collections.deque()
        self._running = 0                      # requests taken by a lane and not yet retired
        self._groups_taken = 0                 # decode groups formed since the pipeline was last idle
        # exclusive: a decode job and an acoustic job never share the chip (each takes this lock for the whole of its GPU work) -- the
        # pipeline then only re-orders and merges the work; measured against the overlapped schedule in profiles/README.md "Round 4"
        if exclusive:
            self._turn = threading.Lock()
        tts.gpt.MAX_WORKSPACES = max(tts.gpt.MAX_WORKSPACES, decode_lanes + 2)

    def submit(self, text_tokens: torch.Tensor, cond, max_mel_tokens: int = 1500, noise: Optional[torch.Tensor] = None,
               repetition_penalty: float = 10.0, sampling: Optional[dict] = None, noise_seed=None,
               takes: int = 1, keep: Optional[int] = None, prefix_codes=None, prefix_logprobs=None, diffusion_steps=None,
               cfg_rate=None) -> concurrent.futures.Future:
        """Queue one batch; returns a Future of the list of waveforms `synthesize_batch` would return.  Inputs produced on the
        caller's current stream are safe to use (an event recorded here is waited for on the lane's stream), and the waveforms
        are safe to read on that stream (they are tied to it with record_stream before the Future resolves).
        noise_seed (instead of `noise`): an int, or one int per row (utterance_noise_seeds) -- the rows' CFM noise seeds are fixed
        here, so the request's noise is the same whatever it is merged with.  A bad value, or both, fails this Future only.
        takes=n > 1 (sampled or beam-sample requests; a greedy one is refused, every take would be the same): the batch is decoded
        with every utterance repeated n times, row i * n + j take j of utterance i, each row drawing its own stream of the request's
        sampler; `noise` and the noise seeds (utterance_noise_seeds(noise_seed, B * n)) have B * n rows, and the Future resolves to
        result[i][j].
        keep=k (1 <= k <= n; sampled, num_beams = 1): the takes are decoded with one prefill per utterance and scored
        (IndexTTS2.ranked_takes: generate(num_return_sequences=n, return_logprobs=True)), and only the best k of every utterance go
        through the latent pass, s2mel and the vocoder: result[i][j], j < k, best first, with their own noise rows / seeds (entry
        i * n + take).  fut.ranking[i] -- every take of utterance i as (take_index, score, stopped, n_codes), best first
        (rank_request) -- is set before the Future resolves.  A request with keep is never merged into another's decode.
        diffusion_steps / cfg_rate: the CFM solver's Euler steps and guidance rate of this request's rows, one value or one per row (B * n
        with takes; acoustic_settings) -- requests with different settings share an acoustic batch under the rules of before, each row
        solved with its own (IndexTTS2.acoustic_stage).  None: the pipeline's tts's values.  A bad value fails this Future only.
        prefix_codes / prefix_logprobs: refused here.  A batch's one-shot decode takes one rectangular prefix, the same k for every
        row, and merges requests by shape; continuing from given codes per utterance is ContinuousPipeline(prefix=True)'s job (or
        UnifiedVoice.generate(input_ids=[fake | codes], prefix_layout="resume") directly)."""
        if prefix_codes is not None or prefix_logprobs is not None:
            raise NotImplementedError("BatchPipeline does not continue from given codes: its one-shot decode takes one rectangular prefix "
                                      "per batch; use ContinuousPipeline(prefix=True).submit(prefix_codes=...)")
        takes = int(takes)
        if takes < 1 or (takes > 1 and not (sampling and sampling.get("do_sample"))):
            raise ValueError("takes must be >= 1, and takes > 1 needs a sampled request: every take of a greedy one would be the same")
        if keep is not None and not (sampling and sampling.get("do_sample")):
            raise ValueError("keep ranks sampled takes: the request must sample (do_sample)")
        keep = _check_keep(keep, takes, True, bool(sampling and int(sampling.get("num_beams") or 1) > 1))
        r = self._new_request(text_tokens, cond, max_mel_tokens, noise, noise_seed, takes, keep, diffusion_steps=diffusion_steps,
                              cfg_rate=cfg_rate)
        if r.done.done():
            return r.done
        r.base = (torch.as_tensor(text_tokens), cond)      # one row per utterance: what a request with keep decodes from
        r.repetition_penalty, r.sampling = repetition_penalty, sampling
        with self._qlock:
            self._queue.append(r)
        self._lanes.submit(self._lane_job)      # one drain per request: a drain that finds the queue empty (its request was merged) returns
        return r.done

    def _take(self):
        with self._qlock:
            if not self._queue:
                return []
            # Slow start: a pipeline that was idle takes its first requests one by one (the first acoustic stage can begin after ONE
            # 16-row decode, 0.6 s, instead of after a merged 48-row one, 1.2-2.3 s with other lanes beside it), then two, then
            # `coalesce` at a time -- the merged decodes' better aggregate rate matters once the acoustic stage is the bottleneck.
            if self._running == 0:
                self._groups_taken = 0
            limit = min(self.coalesce, 1 + self._groups_taken // self.decode_lanes)
            self._drop_cancelled_head()
            if not self._queue:
                return []
            group = [self._queue.popleft()]
            while len(group) < limit and self._drop_cancelled_head() and group[0].compatible(self._queue[0]) and \
                    self._keeps_kernels(group + [self._queue[0]]):
                group.append(self._queue.popleft())
            self._groups_taken += 1
            self._running += len(group)
            return group

    def _drop_cancelled_head(self) -> bool:
        """Drops the cancelled requests at the head of the queue (under _qlock); is a request left?"""
        while self._queue and _cancelled(self._queue[0]):
            self._queue.popleft()
        return bool(self._queue)

    def cancel(self, fut: concurrent.futures.Future) -> bool:
        """fut.cancel(), and the request leaves the queues now.  True: the request is cancelled -- it is never merged into a decode
        group or an acoustic batch from here on (a static decode that has started runs to its end: there is no slot to free, its rows
        are dropped behind it).  False: its acoustic job has started (or it is done) and it completes as usual.  Calling fut.cancel()
        alone has the same outcome; the request is then dropped where the pipeline next touches it."""
        ok = fut.cancel()
        with self._qlock:
            self._queue = collections.deque(r for r in self._queue if not _cancelled(r))
            kept = collections.deque(r for r in self._aq if not _cancelled(r))
            self._running -= len(self._aq) - len(kept)
            self._aq = kept
        return ok

    def _keeps_kernels(self, group) -> bool:
        from . import _lib
        g = self.tts.cfg.gpt
        prefix = g.cond_latents + 2 + int(group[0].text.shape[1]) + 2 + 1      # [cond | start, text, stop] + start_mel (gpt.py::prepare_gpt_inputs)
        return merge_keeps_kernels([r.text.shape[0] for r in group], prefix, _lib.get_gemm_mode() == _lib.GEMM_BF16X3,
                                   self.tts.gpt.weight_format != "f32", _lib.get_decode_plane_rows(),
                                   batch_invariant=bool(getattr(self.tts.gpt, "batch_invariant", False)))

    def _lane_job(self):
        group = self._take()
        if not group:
            return
        handed = 0
        try:
            torch.cuda.set_device(self.device)
            t0 = time.perf_counter()
            sg = self._stream("decode")
            for r in group:
                sg.wait_event(r.ready)
            text = group[0].text if len(group) == 1 else torch.cat([torch.as_tensor(r.text).cpu() for r in group])      # equal widths
            subs = []
            with self._turn, torch.cuda.stream(sg):
                if group[0].keep is not None:      # (a sampled request: alone in its group) every take decoded and ranked, the best kept
                    r = group[0]
                    codes, ranking = self.tts.ranked_takes(r.base[0], r.base[1], r.takes, max_mel_tokens=r.max_mel_tokens,
                                                           repetition_penalty=r.repetition_penalty, sampling=r.sampling)
                    rows = _keep_best(r, ranking, r.keep)
                    r.done.ranking = ranking
                    text = r.text
                    st = self.tts.gpt_stage(text, r.cond, max_mel_tokens=r.max_mel_tokens, repetition_penalty=r.repetition_penalty,
                                            codes=codes[rows])
                else:
                    st = self.tts.gpt_stage(text, group[0].cond, max_mel_tokens=group[0].max_mel_tokens,
                                            repetition_penalty=group[0].repetition_penalty, sampling=group[0].sampling)
                # every request's rows as its own state, cut on the LANE's stream: the slicing copies below are launches like any
                # other, and the acoustic worker reads their results on a stream of its own -- they must be inside what the
                # host-side wait below covers (and allocated from this stream's pool)
                a = 0
                for r in group:
                    b = a + int(r.text.shape[0])
                    n = max(st["code_lens"][a:b])
                    subs.append({"cond": st["cond"], "B": b - a, "codes": st["codes"][a:b, :n].contiguous(), "code_lens": st["code_lens"][a:b],
                                 "code_lens_t": st["code_lens_t"][a:b].clone(), "latent": st["latent"][a:b, :n].contiguous(),
                                 "times": dict(st["times"])})
                    a = b
                # The lane waits for its own stream on the host (the decode has synchronised already, what is left is the latent
                # pass and the slices): a device-side event wait from the acoustic stream is not an option -- HIP refuses to wait on an
                # event whose stream is capturing, and this lane may be capturing the next batch's decode step by then.
                sg.synchronize()
            if self.trace is not None:
                self.trace.append(("decode", t0, time.perf_counter(), int(text.shape[0])))
            for r, sub in zip(group, subs):      # every request's rows go to its own acoustic job; a cancelled one is retired here
                with self._qlock:
                    keep = not _cancelled(r)
                    if keep:
                        r.state = sub
                        self._aq.append(r)
                    else:
                        self._running -= 1
                handed += 1
                if keep:
                    self._acoustic.submit(self._acoustic_drain)      # one drain per request: a drain that finds nothing (merged away) returns
        except BaseException as e:                  # noqa: BLE001 -- handed to the callers through their futures
            with self._qlock:
                self._running -= len(group) - handed      # (requests already handed on or dropped are retired there)
            for r in group:
                _set_exception(r.done, e)

    def _take_acoustic(self):
        """Up to `acoustic_coalesce` decoded requests of one prompt (of any prompts with acoustic_mix_prompts), each with its own CFM
        noise or all with noise seeds (a merged draw from torch's generator would consume it differently from the separate calls).
        The point of no return: every request taken is marked running (_start), so cancel() on it fails from here on; the cancelled
        ones are dropped and retired.  (Merging measured neutral at configs[2]: 181.8 vs 182.3 audio-s/s, profiles/README.md "Round 3";
        useful where single requests are small.)"""
        with self._qlock:
            while self._aq:
                group = [self._aq.popleft()]
                kind = _noise_kind(group[0])
                while (len(group) < self.acoustic_coalesce and self._aq and kind and _noise_kind(self._aq[0]) == kind
                       and (self.acoustic_mix_prompts or self._aq[0].cond is group[0].cond)):
                    group.append(self._aq.popleft())
                kept = [r for r in group if _start(r)]
                self._running -= len(group) - len(kept)
                if kept:
                    return kept
            return []

    def _acoustic_state(self, r: _Request) -> dict:
        return r.state                          # (computed on the lane)

    def _retire(self, group) -> None:
        with self._qlock:
            self._running -= len(group)

    def close(self):
        self._lanes.shutdown(wait=True)
        self._close_acoustic()


_SAMPLING_KEYS = {"do_sample", "num_beams", "temperature", "top_k", "top_p", "sampler", "generator", "seed", "length_penalty"}


def _sampling_params(s: dict, warpers: bool = True, beam: bool = False, check: bool = True) -> tuple:
    """(temperature, top_k, top_p, length_penalty) of a sampling dict: missing (or None) values take UnifiedVoice.generate's and
    generate_beam's defaults, 1.0, 50, 1.0 and 1.0.  `check` (a request that draws): ValueError outside gpt.check_sampling's ranges --
    sampler="accel" runs no warpers, so its top_k / top_p are not looked at; a beam request's top_k is at most 1024 always."""
    from .gpt import check_sampling
    t = float(s["temperature"]) if s.get("temperature") is not None else 1.0
    k = int(s["top_k"]) if s.get("top_k") is not None else 50
    p = float(s["top_p"]) if s.get("top_p") is not None else 1.0
    lp = float(s["length_penalty"]) if s.get("length_penalty") is not None else 1.0
    if check:
        check_sampling(t, k, p, warpers, beam)
    return t, k, p, lp


def utterance_samplers(sampling: Optional[dict], n: int) -> list:
    """The per-utterance samplers of a ContinuousPipeline request (DecodeSession.admit's `sampling` entries).  `sampling` is the dict
    gpt_stage / BatchPipeline take (do_sample, temperature, top_k, top_p, sampler, generator) plus `seed`; missing values take
    UnifiedVoice.generate's defaults (temperature 1.0, top_k 50, top_p 1.0).  Greedy (no dict, or do_sample false): {"sampler":
    "greedy"} for every utterance.  Sampled: utterance i gets seed torch.randint(0, 2**62, (1,), generator=g), drawn in utterance
    order, with g = torch.Generator().manual_seed(seed) when `seed` is given, else the request's `generator`, else torch's global RNG.
    Raises ValueError on a bad parameter."""
    s = dict(sampling or {})
    unknown = set(s) - _SAMPLING_KEYS
    if unknown:
        raise ValueError(f"sampling: unknown keys {sorted(unknown)}")
    if int(s.get("num_beams") or 1) > 1:
        raise ValueError("ContinuousPipeline does not run beam search (num_beams > 1); use BatchPipeline")
    if not s.get("do_sample"):
        return [{"sampler": "greedy"} for _ in range(n)]
    kind = s.get("sampler") or "hf"
    if kind not in ("hf", "accel"):
        raise ValueError("sampler must be 'hf' or 'accel'")
    t, k, p, _ = _sampling_params(s, warpers=kind == "hf")
    return [{"sampler": kind, "temperature": t, "top_k": k, "top_p": p, "seed": sd} for sd in _draw_seeds(n, s.get("seed"), s.get("generator"))]


_BEAM_KEYS = {"do_sample", "num_beams", "temperature", "top_k", "top_p", "generator", "seed", "length_penalty"}


def utterance_beams(sampling: Optional[dict], n: int, num_beams: int) -> list:
    """The per-utterance beam parameters of a request to a num_beams > 1 ContinuousPipeline (BeamDecodeSession.admit's `beam` entries).
    `sampling` is the dict IndexTTS2.infer builds for beams (do_sample, num_beams, temperature, top_k, top_p, length_penalty,
    generator) plus `seed`; num_beams must equal the pipeline's, missing values take UnifiedVoice.generate_beam's defaults (temperature
    1.0, top_k 50, top_p 1.0, length_penalty 1.0; early_stopping False).  Beam-sample (do_sample): utterance i gets its seed by
    utterance_samplers' rule -- torch.randint(0, 2**62, (1,), generator=g) in utterance order, g from `seed`, else `generator`, else
    torch's global RNG.  Raises ValueError on a bad parameter."""
    s = dict(sampling or {})
    unknown = set(s) - _BEAM_KEYS
    if unknown:
        raise ValueError(f"sampling: unknown keys {sorted(unknown)}")
    nb = int(s.get("num_beams") or 1)
    if nb != int(num_beams):
        raise ValueError(f"this ContinuousPipeline runs num_beams={num_beams}; the request asks for num_beams={nb}")
    do_sample = bool(s.get("do_sample"))
    t, k, p, lp = _sampling_params(s, beam=True, check=do_sample)
    seeds = _draw_seeds(n, s.get("seed"), s.get("generator")) if do_sample else [0] * n      # (no draws: no seeds taken)
    return [{"do_sample": do_sample, "temperature": t, "top_k": k, "top_p": p, "length_penalty": lp, "early_stopping": False, "seed": sd}
            for sd in seeds]


class ContinuousPipeline(_Pipeline):
    """Continuous (iteration-level) batching of the GPT decode: each of `decode_lanes` lanes owns one decode session of `slots` rows
    (`UnifiedVoice.decode_session`) on its own stream and host thread.  A lane admits waiting utterances into its free slots --
    utterances of different requests, prompts and text widths share a session -- steps `poll_steps` steps at a time and collects
    the rows that have finished (stop token or the request's own `max_mel_tokens`), so a short row no longer holds its slot while
    the longest row of a static batch runs on.  Once every row of a request is decoded, the request goes through the existing
    path behind the decode: `gpt_stage(text, cond, codes=...)` (trim + latent pass) and `acoustic_stage` on an acoustic worker.

    Greedy, unless allow_sampling: then the sessions are sampled (decode_session(sampled=True)) and submit(sampling=...) takes the
    dict gpt_stage / BatchPipeline take, plus `seed` (utterance_samplers: the per-utterance seeds are fixed at submit, so a request's
    codes are reproducible whatever else is in flight; with submit(noise_seed=...) -- utterance_noise_seeds, fixed at submit too -- so
    is its CFM noise, and with both its audio).  A request's codes equal, bit for bit, row 0 of `UnifiedVoice.generate` on
    `slots` copies of each of its utterances (gpt.DecodeSession; sampled: with that utterance's sampler and seed), whatever else
    shares the session; they can differ from `BatchPipeline` / `synthesize_batch` results, whose decode batch is the request itself
    (the decode attention's key split and the decode GEMV are chosen by row count).  With the GPT in the batch-invariant mode
    (IndexTTS2(batch_invariant=True) / UnifiedVoice.set_batch_invariant, before the pipeline is built) the contract is simply: an
    utterance's codes equal those of `UnifiedVoice.generate` on that utterance alone -- for every `slots`, every lane, and the same
    as `BatchPipeline` and `synthesize_batch` give it under the same seed.  An error (say, a bad token id or a bad sampling
    parameter) fails the offending request's Future only; num_beams > 1 is refused at submit.

    num_beams > 1: beam search / beam-sample.  The lanes own beam sessions (`UnifiedVoice.beam_session`): `slots` rows = slots /
    num_beams groups, one utterance per group, each retiring on its own; submit(sampling=...) takes the dict IndexTTS2.infer builds for
    beams (its num_beams must equal the pipeline's) plus `seed` (utterance_beams).  An utterance's codes equal row 0 of
    `UnifiedVoice.generate_beam` on slots / num_beams copies of it (gpt.BeamDecodeSession).

    acoustic_coalesce > 1: a free acoustic worker takes up to that many decoded requests -- of any prompts -- and runs their s2mel +
    vocoder as ONE batch of at most `acoustic_max_rows` rows (a request with more rows runs alone), then hands every request its own
    rows.  Each request's latent pass (`gpt_stage(codes=)`) still runs on its own: it left-pads the text, so merging it would move
    tile boundaries.  Only requests that carry explicit `noise`, or only requests with a `noise_seed`, are merged -- the two kinds not
    with each other, and a request with neither runs alone (BatchPipeline's rule: a merged draw would consume torch's generator
    differently); the rows of requests with different prompts go through the mixed-prompt CFM (S2Mel.cfm_rows).  A failure
    fails every request of its merged batch and nothing else.  Requests that finish in the same poll are queued together, so a worker
    that is free then sees all of them.  `trace`: set it to a list to record ("acoustic", start, end, rows, request numbers) for
    every acoustic job (host perf_counter times; requests numbered from 0 in submission order).

    Cancellation: the Future is the interface.  fut.cancel() (or pipe.cancel(fut), which also wakes the lanes) succeeds until the
    request's acoustic job starts; from then on it returns False and the request completes.  A cancelled request is dropped wherever
    the pipeline next touches it: its waiting utterances are never admitted, its decoding rows are evicted at the next poll
    (session.evict: their slots or groups are admissible in that same poll), its finished rows are not kept, and it never reaches an
    acoustic job -- the other requests of a merged acoustic batch get their own results.  The rows of a request that failed are
    evicted the same way.  submit(deadline_s=...) cancels a request that many seconds after submit unless its acoustic job has
    started.  Nobody else's codes move (the session contract holds across evictions).

    Priorities: submit(priority=n), larger is more urgent.  The waiting utterances are admitted by (higher priority first, then
    submission order, then utterance index): with every priority equal, in arrival order.  preempt=True lets an urgent request take a
    slot that is in use.  In each poll, after evicting gone requests and before admitting, a lane whose slots are all taken looks at
    the waiting utterances in order: for each one that is strictly more urgent than the least urgent row still decoding here, it parks
    that row (session.park: the row's KV and state gathered into a ParkedRow, bytes proportional to its length, its slot free at once)
    and admits the utterance in its place in the same poll -- the row of lowest priority first, among equals the one admitted last,
    and never more rows than there are more-urgent utterances waiting.  A parked row waits ahead of the never-admitted utterances of
    its own priority; when its turn comes, whichever lane has a free slot resumes it (session.resume: no prefill), and it goes on to
    the codes of its uninterrupted run, bit for bit.  Equal priority never preempts, so nothing ping-pongs.  park_to="host" moves
    every parked row to pinned host memory until it resumes.  A lane does not look at the other lanes' free slots before it parks.  A
    parked request that is cancelled, past its deadline or failed is dropped when next touched; a resume that fails fails that
    request only; close() drains parked rows like any other waiting work.  Strict priorities can starve: a steady stream of urgent
    requests keeps less urgent ones waiting (or parked) for as long as it lasts -- there is no aging.  `trace` also records
    ("park", t, request, utterance) and ("resume", t, request, utterance).

    preempt_groups=True is the same for a beam pipeline (num_beams > 1; preempt=True keeps refusing one, and preempt_groups refuses
    num_beams == 1): the unit that steps aside is a whole group (session.park_group: the request's beams, scorer state and KV -- the
    prompt positions once, the generated ones per beam -- in a ParkedGroup; session.resume_group puts it into a free group of any
    lane), under the same rules: strictly more urgent only, the least urgent and last admitted group first, parked groups ahead of
    never-admitted utterances of their priority, park_to, the trace entries, cancellation, deadlines, failures and close().

    scores=True (num_beams == 1): the sessions record every code's log-probability (decode_session(scores=True)) and
    submit(takes=n, keep=k) ranks each utterance's takes once all of them are decoded; only the best k go on to the latent pass and the
    acoustic job (see submit).  The codes are those of a pipeline without scores.

    prefix_scores=True (with prefix=True and scores=True): submit(prefix_codes=..., prefix_logprobs="model") has the admission's own
    prefill score the given codes (decode_session(prefix_scores=True)), so a re-take ranks with a complete sequence score.

    session_factory(max_prompt, max_new) -> session (admit / step / take / free_slots / close; scores=True: take(slot, scores=True)
    -> (codes, logprobs); evict to cancel; park / resume to
    preempt; a beam pipeline's: free_groups, park_group / resume_group) replaces the HIP session (tests)."""

    def __init__(self, tts, slots: int = 16, decode_lanes: int = 1, acoustic_workers: int = 1, poll_steps: int = 16,
                 repetition_penalty: float = 10.0, max_prompt: Optional[int] = None, max_new: Optional[int] = None,
                 session_factory=None, allow_sampling: bool = False, num_beams: int = 1, acoustic_coalesce: int = 1,
                 acoustic_max_rows: int = 16, preempt: bool = False, park_to: str = "device", preempt_groups: bool = False,
                 scores: bool = False, prefix: bool = False, prefix_scores: bool = False):
        if slots < 1 or decode_lanes < 1 or acoustic_workers < 1 or poll_steps < 1 or acoustic_coalesce < 1 or acoustic_max_rows < 1:
            raise ValueError("slots, decode_lanes, acoustic_workers, poll_steps, acoustic_coalesce and acoustic_max_rows must be >= 1")
        self._cv = threading.Condition()
        super().__init__(tts, acoustic_workers, self._cv, cuda=torch.device(tts.device).type == "cuda")
        self.acoustic_coalesce, self.acoustic_max_rows = int(acoustic_coalesce), int(acoustic_max_rows)
        self._submitted = 0
        self._clock = time.monotonic            # deadlines are read off this clock
        self.num_beams = int(num_beams)
        if not 1 <= self.num_beams <= 8:
            raise ValueError("num_beams must be in 1 .. 8")
        if slots % self.num_beams:
            raise ValueError(f"slots ({slots}) must be a multiple of num_beams ({self.num_beams})")
        g = tts.cfg.gpt
        self.slots, self.poll_steps, self.repetition_penalty = slots, poll_steps, float(repetition_penalty)
        self.max_prompt = int(max_prompt or g.cond_latents + 2 + g.max_text_tokens + 2)      # [cond | start, text, stop]
        self.max_new = int(max_new or g.max_mel_tokens)
        self.allow_sampling = bool(allow_sampling)
        self.scores = bool(scores)
        if self.scores and self.num_beams > 1:
            raise ValueError("scores=True needs num_beams == 1: a beam pipeline's takes are the scorer's n best, already ranked")
        self.preempt = bool(preempt)
        if park_to not in ("device", "host"):
            raise ValueError('park_to must be "device" or "host"')
        self.park_to = park_to
        if self.preempt and self.num_beams > 1:
            raise ValueError("preempt=True needs num_beams == 1: a beam pipeline parks whole groups (preempt_groups=True)")
        self.preempt_groups = bool(preempt_groups)
        if self.preempt_groups and self.num_beams == 1:
            raise ValueError("preempt_groups=True needs num_beams > 1: a greedy or sampled pipeline parks rows (preempt=True)")
        self._preempts = self.preempt or self.preempt_groups      # rows or groups: the scheduling is the same
        self.prefix = bool(prefix)
        if self.prefix and self.num_beams > 1:
            raise ValueError("prefix=True needs num_beams == 1: beams do not continue from given codes")
        self.prefix_scores = bool(prefix_scores)
        if self.prefix_scores and not (self.prefix and self.scores):
            raise ValueError("prefix_scores=True needs prefix=True and scores=True")
        self._admitted = 0                      # admission stamps (which row of a priority was admitted last)
        if self.num_beams > 1:
            self._factory = session_factory or (lambda mp, mn: tts.gpt.beam_session(slots, self.num_beams, mp, mn,
                                                                                   repetition_penalty=self.repetition_penalty))
        else:
            self._factory = session_factory or (lambda mp, mn: tts.gpt.decode_session(
                slots, mp, mn, repetition_penalty=self.repetition_penalty, sampled=self.allow_sampling, **({"scores": True} if self.scores else {}),
                **({"prefix": True} if self.prefix else {}), **({"prefix_scores": True} if self.prefix_scores else {})))
        self._waiting = collections.deque()     # (job, utterance index, ParkedRow or None) waiting for a slot, most urgent first
        self._closing = False
        self._alive = decode_lanes
        self._lanes = [threading.Thread(target=self._lane, name=f"idxtts-session-{i}", daemon=True) for i in range(decode_lanes)]
        for t in self._lanes:
            t.start()

    def submit(self, text_tokens: torch.Tensor, cond, max_mel_tokens: int = 1500, noise: Optional[torch.Tensor] = None,
               repetition_penalty: float = 10.0, sampling: Optional[dict] = None, noise_seed=None,
               deadline_s: Optional[float] = None, priority: int = 0, takes: int = 1,
               keep: Optional[int] = None, prefix_codes=None, prefix_logprobs=None, diffusion_steps=None,
               cfg_rate=None) -> concurrent.futures.Future:
        """BatchPipeline.submit's contract (a Future of the list of waveforms; noise_seed, diffusion_steps and cfg_rate as there); max_mel_tokens caps each row.  sampling: greedy
        only, unless the pipeline was built with allow_sampling (see utterance_samplers); a num_beams > 1 pipeline takes beam requests
        (see utterance_beams).  deadline_s: seconds from now after which the pipeline cancels the request, unless its acoustic job
        has started by then (checked wherever cancellation is: each poll, each acoustic hand-over); None: no deadline.
        priority: larger is more urgent (see the class); it orders the waiting utterances and, with preempt=True, lets this request
        park rows of lower priority.
        takes=n > 1: n takes of every utterance; the Future resolves to result[i][j], take j of utterance i (takes=1: the flat list).
        Sampled pipelines: utterance i, take j gets entry i * n + j of utterance_samplers(sampling, B * n) and of
        utterance_noise_seeds(noise_seed, B * n) (`noise`: B * n rows); the takes are ordinary rows for admission order, cancellation,
        deadlines, priorities, park and resume, and the takes of an utterance that are admitted in one poll share one prefill
        (DecodeSession.admit(takes=)) -- a request whose takes do not all fit is admitted in parts.  Greedy requests are refused
        (every take would be the same).  Beam pipelines: the n best hypotheses of each utterance's group
        (BeamDecodeSession.take(n_best=)), n <= num_beams, else the request's Future fails; the noise seeds are again B * n.
        keep=k (1 <= k <= n; a pipeline built with scores=True, a sampled request): once every take of the request is decoded, each
        utterance's takes are ranked (rank_request: stopped takes first, then the higher sequence score of the codes' log-probabilities,
        then the lower take index), and only the best k go to gpt_stage(codes=) and the acoustic job.  The Future resolves to
        result[i][j], j < k, best first; before that, fut.ranking[i] is set: all n takes of utterance i as (take_index, score, stopped,
        n_codes), best first.  Noise rows and seeds follow the kept takes (take j keeps entry i * n + j).  Every take still decodes to
        its end and is an ordinary row for cancellation, deadlines, priorities, park and resume; a cancelled request is never ranked.
        keep=None: every take is synthesised, as ever.  keep without scores=True, or on a beam pipeline, raises ValueError here.
        prefix_codes (a pipeline built with prefix=True; greedy or sampled): one 1-D sequence of mel codes, or None, per utterance --
        the utterance is decoded on from behind them as the row that produced them would have gone on (DecodeSession.admit(prefix=)).
        With takes=n the n takes of an utterance share its prefix and one prefill; max_mel_tokens caps prefix + continuation; the codes
        that go to gpt_stage(codes=) and the acoustic job are prefix + continuation.  prefix_logprobs (scores=True): one fp32 sequence
        or None per utterance; with keep= the ranking uses the recorded log-probabilities, which for the prefix codes are these values,
        or 0 where none are given -- takes of one utterance share them, so their order is decided by the continuations.  The string
        "model" (for one utterance, or for every one that has a prefix; a pipeline built with prefix_scores=True) has the admission's
        prefill compute them: the sequence score then counts every code, as a take decoded from the start does.  Refused here
        (ValueError): a beam pipeline, a pipeline built without prefix=True, a prefix that holds the stop token or a code outside the
        table, or one that is not shorter than max_mel_tokens."""
        pfx = self._check_prefix(text_tokens, prefix_codes, prefix_logprobs, int(max_mel_tokens))
        if deadline_s is not None:
            deadline_s = float(deadline_s)
        priority, takes = int(priority), int(takes)
        if takes < 1:
            raise ValueError("takes must be >= 1")
        keep = _check_keep(keep, takes, self.scores, self.num_beams > 1)
        if keep is not None and not (self.allow_sampling and sampling and sampling.get("do_sample")):
            raise ValueError("keep ranks sampled takes: the request must sample (allow_sampling, do_sample)")
        beam = self.num_beams > 1
        if not beam:
            if sampling and not self.allow_sampling:
                raise ValueError("this ContinuousPipeline decodes greedily; build it with allow_sampling=True (or use BatchPipeline) to sample")
            if sampling and int(sampling.get("num_beams") or 1) > 1:
                raise ValueError("ContinuousPipeline does not run beam search (num_beams > 1); use BatchPipeline")
            if takes > 1 and not (self.allow_sampling and sampling and sampling.get("do_sample")):
                raise ValueError("takes > 1 needs a sampled request: every take of a greedy one would be the same")
        if float(repetition_penalty) != self.repetition_penalty:
            raise ValueError(f"this pipeline's sessions use repetition_penalty={self.repetition_penalty}")
        if not 1 <= int(max_mel_tokens) <= self.max_new:
            raise ValueError(f"max_mel_tokens must be in 1 .. {self.max_new}")

        def samplers(rows: int):                # a bad parameter fails this request's Future only
            if not beam:
                return utterance_samplers(sampling, rows) if self.allow_sampling else None
            if takes > self.num_beams:
                raise ValueError(f"takes ({takes}) exceeds the pipeline's num_beams ({self.num_beams})")
            per = utterance_beams(sampling, rows // takes, self.num_beams)
            return [per[r // takes] for r in range(rows)]

        # takes: the request holds one row per take, row i * takes + j (text and conditioning repeated).  A sampled pipeline decodes every
        # row; a beam pipeline decodes one group per utterance, queued as the utterance's first row, and reads its `takes` best
        j = self._new_request(text_tokens, cond, int(max_mel_tokens), noise, noise_seed, takes, keep, samplers, diffusion_steps, cfg_rate)
        if j.done.done():
            return j.done
        B = int(j.text.shape[0])
        j.nbest = takes if beam else 1
        # prefixes: one entry per row (the takes of an utterance share theirs)
        j.prefix = None if pfx is None else [pfx[0][r // takes] for r in range(B)]
        j.prefix_lps = None if pfx is None else [pfx[1][r // takes] for r in range(B)]
        j.codes, j.left, j.failed = [None] * B, B // j.nbest, False
        j.lps = None if keep is None else [None] * B
        j.priority, j.stamp = priority, [0] * B
        j.deadline = None if deadline_s is None else self._clock() + deadline_s
        with self._cv:
            if self._closing or self._alive == 0:
                raise RuntimeError("pipeline closed" if self._closing else "every decode lane has failed")
            j.seq = self._submitted
            self._submitted += 1
            for i in range(0, B, j.nbest):
                self._enqueue(j, i, None)
            self._cv.notify_all()
        return j.done

    def _check_prefix(self, text_tokens, prefix_codes, prefix_logprobs, max_mel_tokens: int):
        """submit(prefix_codes=, prefix_logprobs=) -> None, or (codes, logprobs): one CPU tensor or None per utterance."""
        if prefix_codes is None and prefix_logprobs is None:
            return None
        if self.num_beams > 1:
            raise ValueError("prefix_codes on a beam pipeline: beams do not continue from given codes")
        if not self.prefix:
            raise ValueError("prefix_codes needs a pipeline built with prefix=True (its sessions size their prefill area for it)")
        if prefix_codes is None:
            raise ValueError("prefix_logprobs without prefix_codes")
        if prefix_logprobs is not None and not self.scores:
            raise ValueError("prefix_logprobs needs a pipeline built with scores=True")
        B = int(torch.as_tensor(text_tokens).shape[0])
        codes = list(prefix_codes)
        if isinstance(prefix_logprobs, str):      # "model" for every utterance that has a prefix
            prefix_logprobs = [None if c is None else prefix_logprobs for c in codes]
        lps = [None] * B if prefix_logprobs is None else list(prefix_logprobs)
        if any(isinstance(l, str) for l in lps):
            if any(isinstance(l, str) and l != "model" for l in lps):
                raise ValueError('prefix_logprobs: a sequence, None or the string "model" per utterance')
            if not self.prefix_scores:
                raise ValueError('prefix_logprobs="model" needs a pipeline built with prefix_scores=True (and prefix=True, scores=True)')
        if len(codes) != B or len(lps) != B:
            raise ValueError("prefix_codes / prefix_logprobs: one entry (a 1-D sequence or None) per utterance")
        from .gpt import check_prefix
        out_c, out_l = [None] * B, [None] * B
        for b, (c, l) in enumerate(zip(codes, lps)):
            if c is None:
                if l is not None:
                    raise ValueError("prefix_logprobs for an utterance without prefix_codes")
                continue
            model = isinstance(l, str)          # (the admission scores the codes: there are no values to check)
            c, given = check_prefix(c, None if model else l, self.tts.cfg.gpt, max_mel_tokens, "prefix_codes")      # max_mel_tokens caps prefix + continuation
            if c.numel():
                out_c[b], out_l[b] = c, l if model else given
        return (out_c, out_l) if any(c is not None for c in out_c) else None

    @staticmethod
    def _order(j: _Request, i: int, parked) -> tuple:
        """Where a waiting entry stands: higher priority first, parked rows ahead of never-admitted utterances of their priority, then
        submission order, then utterance index."""
        return (-j.priority, parked is None, j.seq, i)

    def _enqueue(self, j: _Request, i: int, parked) -> None:
        """Puts an entry into the waiting queue at its place (self._cv held); with every priority equal that is the end."""
        key, at = self._order(j, i, parked), len(self._waiting)
        while at > 0 and self._order(*self._waiting[at - 1]) > key:
            at -= 1
        self._waiting.insert(at, (j, i, parked))

    def cancel(self, fut: concurrent.futures.Future) -> bool:
        """fut.cancel(), and the lanes are woken so that the request is dropped at once.  True: the request is cancelled (see the
        class); False: its acoustic job has started (or it is done) and it completes as usual."""
        ok = fut.cancel()
        with self._cv:
            self._cv.notify_all()
        return ok

    def _gone(self, j: _Request) -> bool:
        """Is there nobody left to decode `j` for -- cancelled (by its caller, or here: past its deadline) or failed?"""
        if j.deadline is not None and not j.done.done() and self._clock() >= j.deadline:
            j.done.cancel()                     # refused once the acoustic job has started: the request then completes
        return j.failed or _cancelled(j)

    def _evict_gone(self, sess, in_slot) -> None:
        """Frees the slots (groups) whose request is gone, in one evict call; sessions without evict are never asked while there is
        nothing to evict."""
        gone = [s for s, (j, _) in in_slot.items() if self._gone(j)]
        if gone:
            sess.evict(gone)
            for s in gone:
                del in_slot[s]

    def _prompt_rows(self, j: _Request, idx):
        """The [P, d] prompts of utterances `idx` of a job (prepare_gpt_inputs, unpadded), on the current stream."""
        self._wait_ready(j)
        c = j.cond.to(self.device)
        lat = c.spk_cond_latent if c.spk_cond_latent.shape[0] == 1 else c.spk_cond_latent[idx]
        emo = c.emo_vec if c.emo_vec.shape[0] == 1 else c.emo_vec[idx]
        conds = self.tts.gpt.conds_latent(lat, emo)
        return self.tts.gpt.prompt_rows(conds, j.text[idx])

    def _free(self, sess):
        """Free places of a lane's session: slots, or groups of a beam session."""
        return sess.free_groups if self.num_beams > 1 else sess.free_slots

    def _admit(self, sess, in_slot) -> None:
        """One poll's admission: choose, make room (park) and resume, build the new rows' admission, hand it to the session."""
        take, victims = self._choose(sess, in_slot)
        for s in victims:                       # their slots are free for `take` in this poll
            self._park(sess, in_slot, s)
        for j, i, parked in take:
            if parked is not None:
                self._resume(sess, in_slot, j, i, parked)
        parts = self._admission([(j, i) for j, i, parked in take if parked is None])
        if not parts:
            return
        owners = [o for p in parts for o in p.owners]
        try:
            got = self._session_admit(sess, parts)
        except BaseException as e:           # noqa: BLE001 -- refused before any slot was taken: these requests fail, the lane goes on
            for j, _ in owners:
                self._fail(j, e)
            return
        with self._cv:
            for s, (j, i) in zip(got, owners):
                in_slot[s] = (j, i)
                self._admitted += 1
                j.stamp[i] = self._admitted

    def _choose(self, sess, in_slot) -> tuple:
        """The waiting entries this poll takes, in order, and the slots whose rows step aside for them: (take, victims)."""
        with self._cv:
            take, victims = [], []
            free = len(self._free(sess))
            # the rows a more urgent utterance may displace, first choice first: lowest priority, among equals admitted last
            rows = sorted(in_slot, key=lambda s: (in_slot[s][0].priority, -in_slot[s][0].stamp[in_slot[s][1]])) if self._preempts else []
            while self._waiting:
                j = self._waiting[0][0]
                room = len(take) < free
                if not room and not (len(victims) < len(rows) and in_slot[rows[len(victims)]][0].priority < j.priority):
                    break
                j, i, parked = self._waiting.popleft()
                if self._gone(j):               # a cancelled or failed request's waiting utterances (and parked rows) are dropped
                    continue
                if not room:
                    victims.append(rows[len(victims)])
                take.append((j, i, parked))
        return take, victims

    def _admission(self, new) -> list:
        """The never-admitted rows (request, row) this poll takes, as one _Part per utterance: the takes of one utterance taken in one
        poll are one request with that many takes -- one prompt, one prefill.  A request whose prompts cannot be built (a bad token
        id, too long) fails, alone."""
        by_job = collections.OrderedDict()
        for j, i in new:
            share = j.takes if self.num_beams == 1 else 1
            by_job.setdefault(id(j), (j, collections.OrderedDict()))[1].setdefault(i // share, []).append(i)
        parts = []
        for j, utts in by_job.values():
            try:
                prompts = self._prompt_rows(j, [p[0] for p in utts.values()])
                if any(int(r.shape[0]) > self.max_prompt for r in prompts):
                    raise ValueError(f"prompt longer than the pipeline's max_prompt ({self.max_prompt})")
            except BaseException as e:       # noqa: BLE001 -- the request's own error
                self._fail(j, e)
                continue
            for prompt, p in zip(prompts, utts.values()):
                parts.append(_Part(prompt, [(j, i) for i in p], [j.max_mel_tokens] * len(p),
                                   None if j.sampling is None else [j.sampling[i] for i in p],
                                   None if j.prefix is None else j.prefix[p[0]], None if j.prefix is None else j.prefix_lps[p[0]]))
        return parts

    def _session_admit(self, sess, parts) -> list:
        """sess.admit in the form the parts need, each passing what it needs and nothing more -> the slots (a beam session: the
        groups), one per row in the parts' order."""
        rows, caps, counts = [p.prompt for p in parts], [p.caps for p in parts], [len(p.owners) for p in parts]
        if any(p.prefix is not None for p in parts):      # some utterance continues from given codes: its takes share the prefix
            kw = {"sampling": [p.samplers for p in parts]} if self.allow_sampling else {}
            if self.scores and any(p.prefix_lps is not None for p in parts):
                kw["prefix_logprobs"] = [p.prefix_lps for p in parts]
            return [s for g in sess.admit(rows, caps, takes=counts, prefix=[p.prefix for p in parts], **kw) for s in g]
        if max(counts) > 1:                     # (sampled pipelines only)
            return [s for g in sess.admit(rows, caps, sampling=[p.samplers for p in parts], takes=counts) for s in g]
        caps = [c[0] for c in caps]
        if self.num_beams > 1:
            return sess.admit(rows, caps, beam=[p.samplers[0] for p in parts])
        if self.allow_sampling:
            return sess.admit(rows, caps, sampling=[p.samplers[0] for p in parts])
        return sess.admit(rows, caps)

    def _park(self, sess, in_slot, s) -> None:
        """Parks the row in slot s (a beam pipeline: the group s) and queues it for whichever lane next has room; a park that fails
        fails its request (and frees the slot by eviction)."""
        j, i = in_slot.pop(s)
        try:
            parked = sess.park_group(s) if self.num_beams > 1 else sess.park(s)
            if self.park_to == "host":
                parked = parked.to("cpu")
        except BaseException as e:           # noqa: BLE001
            self._fail(j, e)
            sess.evict([s])
            return
        if self.trace is not None:
            self.trace.append(("park", time.perf_counter(), j.seq, i))
        with self._cv:
            self._enqueue(j, i, parked)
            self._cv.notify_all()

    def _resume(self, sess, in_slot, j: _Request, i: int, parked) -> None:
        try:
            s = sess.resume_group(parked) if self.num_beams > 1 else sess.resume(parked)
        except BaseException as e:           # noqa: BLE001 -- this request's own failure: nothing was changed, the lane goes on
            self._fail(j, e)
            return
        in_slot[s] = (j, i)
        if self.trace is not None:
            self.trace.append(("resume", time.perf_counter(), j.seq, i))

    def _collect(self, sess, in_slot, finished) -> None:
        done = []
        for s in finished:
            j, i = in_slot.pop(s)
            if j.nbest > 1:                     # a beam group's n best: the rows i .. i + n - 1 of the job
                best = [c.cpu() for c, _ in sess.take(s, n_best=j.nbest)]
            elif self.scores:                   # a scored session: the codes' log-probabilities come with them
                c, lp = sess.take(s, scores=True)
                best = [c.cpu()]
                if j.lps is not None:
                    j.lps[i] = lp.cpu()
            else:
                best = [sess.take(s).cpu()]
            if self._gone(j):
                continue
            j.codes[i:i + len(best)] = best
            j.left -= 1
            if j.left == 0:
                if j.keep is not None:          # every take is decoded: rank them, the best `keep` of each utterance go on
                    ranking = rank_request(j.codes, j.lps, j.takes, self.tts.cfg.gpt.stop_mel_token)
                    rows = _keep_best(j, ranking, j.keep)
                    j.codes, j.lps = [j.codes[q] for q in rows], None
                    j.done.ranking = ranking
                done.append(j)
        if done:
            with self._cv:                  # every request this poll finished is queued before any worker looks
                self._aq.extend(done)
            for _ in done:
                self._acoustic.submit(self._acoustic_drain)      # one drain per request: a drain that finds nothing (merged away) returns

    def _lane(self):
        sess, in_slot = None, {}
        try:
            if self._cuda:
                torch.cuda.set_device(self.device)
            stream = self._stream("decode")
            with self._on(stream):
                sess = self._factory(self.max_prompt, self.max_new)
                while True:
                    with self._cv:
                        while not self._waiting and not in_slot and not self._closing:
                            self._cv.wait()
                        if self._closing and not self._waiting and not in_slot:
                            break
                    self._evict_gone(sess, in_slot)      # before admitting: the freed places are admissible in this poll
                    if self._free(sess) or (self._preempts and in_slot):
                        self._admit(sess, in_slot)
                    if in_slot:
                        self._collect(sess, in_slot, sess.step(self.poll_steps))
        except BaseException as e:              # noqa: BLE001 -- a session failure: the requests in its slots fail (and the waiting
            pending = list(in_slot.values())    # ones too when no other lane is left to take them)
            with self._cv:
                self._alive -= 1
                if self._alive == 0:
                    pending += list(self._waiting)
                    self._waiting.clear()
            for j, *_ in pending:
                self._fail(j, e)
            return
        finally:
            if sess is not None:
                sess.close()
        with self._cv:
            self._alive -= 1

    def _take_acoustic(self) -> list:
        """The next acoustic job: the oldest decoded request, plus -- when it carries explicit noise, or noise seeds -- the next ones of
        the same kind, up to `acoustic_coalesce` requests and `acoustic_max_rows` rows (requests with neither, of the other kind, or with
        too many rows, wait for a job of their own).  Requests that are gone are dropped from the queue first.  The point of no return:
        every request taken is marked running (_start), so cancel() on it fails from here on."""
        with self._cv:
            while True:
                self._aq = collections.deque(j for j in self._aq if not self._gone(j))
                if not self._aq:
                    return []
                group = [self._aq.popleft()]
                rows = int(group[0].text.shape[0])
                kind = _noise_kind(group[0])
                if kind:
                    i = 0
                    while len(group) < self.acoustic_coalesce and i < len(self._aq):
                        j = self._aq[i]
                        nb = int(j.text.shape[0])
                        if _noise_kind(j) == kind and rows + nb <= self.acoustic_max_rows:
                            del self._aq[i]
                            group.append(j)
                            rows += nb
                        else:
                            i += 1
                group = [j for j in group if _start(j)]      # (but for a cancel that landed since the check above)
                if group:
                    return group

    def _acoustic_state(self, j: _Request) -> dict:
        """The latent pass of a decoded request, on the acoustic worker (per request: merging it would re-pad the text)."""
        n = max(int(c.shape[0]) for c in j.codes)
        codes = torch.full((len(j.codes), n), self.tts.cfg.gpt.stop_mel_token, dtype=torch.long)
        for i, c in enumerate(j.codes):
            codes[i, : c.shape[0]] = c
        self._wait_ready(j)
        return self.tts.gpt_stage(j.text, j.cond, max_mel_tokens=j.max_mel_tokens, repetition_penalty=self.repetition_penalty, codes=codes)

    def _acoustic_entry(self, t0: float, t1: float, rows: int, group) -> tuple:
        return ("acoustic", t0, t1, rows, tuple(j.seq for j in group))

    def close(self):
        with self._cv:
            self._closing = True
            self._cv.notify_all()
        for t in self._lanes:
            t.join()
        self._close_acoustic()
