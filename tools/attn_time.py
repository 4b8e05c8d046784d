"""Per-launch time of the DiT planes attention at the bench shape (B = 32 with CFG -> 64 rows, T = 1130, prompt 689), by the library's own
per-launch HIP events: `python tools/attn_time.py [windows]` on a GPU box.  Every `flash_attn_*` category the profile holds is reported:
the mean per launch of each window (one estimator call) and the median of the windows."""
import statistics, sys, torch
sys.path.insert(0, "index-tts_amd")
from indextts_amd import weights, _lib
from indextts_amd.config import PipelineConfig
from indextts_amd.s2mel import S2Mel
windows = int(sys.argv[1]) if len(sys.argv) > 1 else 5
dev = torch.device("cuda", 0)
cfg = PipelineConfig()
sm = S2Mel(weights.synth_s2mel_weights(cfg.s2mel, tag="bench/s2mel"), cfg.s2mel, device=dev)
B, Tp, T = 32, 689, 1130
C = cfg.s2mel.in_channels
x = torch.randn(B, C, T, device=dev); px = torch.zeros(B, C, T, device=dev); px[..., :Tp] = torch.randn(B, C, Tp, device=dev)
st = torch.randn(B, cfg.s2mel.style_dim, device=dev); mu = torch.randn(B, T, cfg.s2mel.content_dim, device=dev); t = torch.full((B,), 0.4)
lens = torch.LongTensor([T] * B)
for _ in range(2): sm.estimator(x, px, lens, t, st, mu)
torch.cuda.synchronize()
us, launches = {}, {}
for _ in range(windows):
    _lib.profile_enable(True)
    sm.estimator(x, px, lens, t, st, mu)
    torch.cuda.synchronize()
    prof = _lib.profile_read(); _lib.profile_enable(False)
    for name, v in prof.items():
        if name.startswith("flash_attn_"):
            us.setdefault(name, []).append(1000 * v["ms"] / v["launches"]); launches[name] = v["launches"]
assert us, "no flash_attn_* launch in the profile"
for name, w in sorted(us.items()):
    print(f"{name}: {launches[name]} launches per window, us each per window {' '.join(f'{u:.1f}' for u in w)}, median {statistics.median(w):.1f}", flush=True)
