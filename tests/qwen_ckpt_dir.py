"""Test helper: a `qwen_emo_path` directory in the layout the reference loads with AutoModelForCausalLM / AutoTokenizer
(infer_v2.py:949-960), written from the synthetic Qwen3 weights at reduced size:

    config.json               the Qwen3Config fields
    model.safetensors         the state dict under the HF keys, BF16 (as the published checkpoint) or F32
    generation_config.json    eos_token_id

plus the stub tokenizer the classifier tests bind in place of transformers' (one id per character; the fixture generator
tests/golden/make_qwen_golden.py uses the same codec)."""
import dataclasses
import json
import os

import numpy as np

from indextts_amd.qwen_emo import QwenConfig, synth_qwen_weights

EOS_ID, THINK_END_ID, CHAR_BASE = 151645, 151668, 1000


def write_safetensors(path, tensors, dtype="BF16"):
    """{name: float32 array} -> a .safetensors file written by hand (8-byte header length, JSON header, raw little-endian data)."""
    header, chunks, off = {}, [], 0
    for name, a in tensors.items():
        shape = list(np.shape(a))      # (ascontiguousarray turns a 0-d array into [1])
        a = np.ascontiguousarray(a, dtype=np.float32)
        if dtype == "BF16":
            u = a.view(np.uint32)
            assert not (u & np.uint32(0xFFFF)).any(), f"{name} is not on the bf16 grid"
            raw = (u >> np.uint32(16)).astype("<u2").tobytes()
        else:
            raw = a.astype("<f4").tobytes()
        header[name] = {"dtype": dtype, "shape": shape, "data_offsets": [off, off + len(raw)]}
        chunks.append(raw)
        off += len(raw)
    header["__metadata__"] = {"format": "pt"}
    hj = json.dumps(header).encode("utf-8")
    hj += b" " * (-len(hj) % 8)
    with open(path, "wb") as f:
        f.write(len(hj).to_bytes(8, "little"))
        f.write(hj)
        for c in chunks:
            f.write(c)


def write_qwen_dir(path, cfg: QwenConfig = None, tag="t/qwen/ckpt", dtype="BF16", eos_ids=(EOS_ID,)):
    cfg = cfg or QwenConfig.tiny()
    os.makedirs(path, exist_ok=True)
    w = synth_qwen_weights(cfg, tag=tag)
    j = {k: v for k, v in dataclasses.asdict(cfg).items() if k != "max_context"}
    j.update(model_type="qwen3", architectures=["Qwen3ForCausalLM"], max_position_embeddings=cfg.max_context)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(j, f)
    with open(os.path.join(path, "generation_config.json"), "w") as f:
        json.dump({"eos_token_id": list(eos_ids), "do_sample": False}, f)
    write_safetensors(os.path.join(path, "model.safetensors"), w, dtype)
    return cfg, w


def encode_text(s):
    return [CHAR_BASE + ord(c) for c in s]


class StubTokenizer:
    """Duck-typed stand-in for the Qwen tokenizer: records every call, one id per character (mod `vocab` when given, so the ids fit a
    reduced model), decode drops the two special ids."""
    eos_token_id = EOS_ID

    def __init__(self, vocab=None):
        self.calls = []
        self.vocab = vocab

    def apply_chat_template(self, messages, **kw):
        self.calls.append(["apply_chat_template", messages, kw])
        return "".join(f"<{m['role']}>{m['content']}" for m in messages) + "<assistant>"

    def __call__(self, texts, **kw):
        self.calls.append(["__call__", texts, kw])
        ids = [encode_text(t) for t in texts]
        if self.vocab:
            ids = [[i % self.vocab for i in row] for row in ids]
        return {"input_ids": ids}

    def decode(self, ids, **kw):
        self.calls.append(["decode", None, kw])
        special = {EOS_ID, THINK_END_ID} if kw.get("skip_special_tokens") else set()
        return "".join(chr(i - CHAR_BASE) if i >= CHAR_BASE else "?" for i in ids if i not in special)
