#!/usr/bin/env python3
"""One sha256 per output of the dense-layer units (csrc/video_query.hip, autoencoder.hip, query.hip) of the
library that LSR_LIBRARY names (default: the tree's build), on seeded inputs at the shapes of the units' GPU
tests.  The kernels have no atomics, so two builds that compute the same sums in the same order print the same
lines: run it once per library, each in a fresh process, and compare the outputs as text.
    LSR_LIBRARY=4dlangsplat_amd/build/variants/liblsr_base.so python tools/dense_digest.py > bits_base.txt
    python tools/dense_digest.py > bits_head.txt
  video   row_cosines at the sweep shapes of tests/test_video_query_gpu.py (video_query_cases.case)
  ae      encode and reconstruction_loss (eval state), and the parameters and both Adam moments after 8
          AutoencoderTrainer.step at autoencoder_cases' fixture, odd-width and CLIP shapes
  query   decode and relevancy at query_cases' default decoder
The library's path is not printed."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "4dlangsplat_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import autoencoder_cases as ac  # noqa: E402
import query_cases as qc  # noqa: E402
import video_query as vq  # noqa: E402
import video_query_cases as vc  # noqa: E402
from language_autoencoder import AutoencoderTrainer, LanguageAutoencoder  # noqa: E402
from language_query import LanguageDecoder, relevancy  # noqa: E402

T = vq.ROW_TILE
NARROW, TALL = [6, 48, 528, 1040], [3, 16, 2064]


def digest(name, t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    print(f"{name} {a.dtype.str}{list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def video():
    cases = [(NARROW, n, 4, 100 + n) for n in (1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 1)]
    cases += [([6] + w, T + 1, 4, 200 + len(w) + w[0]) for w in ([16], [4096], [48, 528], [1040, 16], [32] * 8)]
    cases += [([c] + NARROW[1:], T + 1, 4, 300 + c) for c in (1, 3, 6, 32)]
    cases += [(TALL, T + 1, n_q, 400 + n_q) for n_q in (1, 2, 8, 16)]
    for dims, n_rows, n_q, seed in cases:
        ws, bs, rows, q = vc.case(dims, n_rows, n_q, seed)
        dec = LanguageDecoder.from_state_dict(vc.state_dict(ws, bs, torch)).to("cuda")
        assert vq.native_ok(dec)
        digest(f"video row_cosines dims={'-'.join(map(str, dims))} rows={n_rows} n_q={n_q}", vq.row_cosines(cuda(rows), dec, cuda(q)))


def autoencoder():
    shapes = {"fixture": ((ac.FEATURE, ac.ENC, ac.DEC), ac.BATCH), "odd": (ac.ODD, 37), "clip": (ac.CLIP, 64)}
    for name, (shape, batch) in shapes.items():
        feature = shape[0]
        ev = LanguageAutoencoder(ac.torch_state_dict(ac.state_dict_np(*shape, 3, running=True), torch)).to(device="cuda")
        assert ev.native_ok()
        x = cuda(ac.unit_rows(2049, feature, 4))
        digest(f"ae {name} encode rows=2049", ev.encode(x))
        for i, v in enumerate(ev.reconstruction_loss(x)):
            digest(f"ae {name} reconstruction_loss[{i}] rows=2049", v)
        ae = LanguageAutoencoder(ac.torch_state_dict(ac.state_dict_np(*shape, 1), torch)).to(device="cuda")
        tr = AutoencoderTrainer(ae, lr=ac.LR, cos_weight=ac.COS_WEIGHT)
        batches = ac.unit_rows(8 * batch, feature, 2).reshape(8, batch, feature)
        for s in range(8):
            losses = tr.step(cuda(batches[s]))
        for i, v in enumerate(losses):
            digest(f"ae {name} step 8 loss[{i}]", v)
        for k in ae.sd:                                        # the BatchNorm buffers too
            digest(f"ae {name} step 8 {k}", ae.sd[k])
        for k in tr.exp_avg:
            digest(f"ae {name} step 8 exp_avg {k}", tr.exp_avg[k])
            digest(f"ae {name} step 8 exp_avg_sq {k}", tr.exp_avg_sq[k])


def query():
    for n_pix, seed in ((129, 100), (1073, 700)):
        ws, bs, lat, pos, neg = qc.case(qc.FIXTURE_DIMS, n_pix, 6, 4, seed)
        dec = LanguageDecoder.from_state_dict(qc.state_dict(ws, bs, torch)).to("cuda")
        x = cuda(lat)[:, None, :]
        digest(f"query decode n_pix={n_pix}", dec.decode(x))
        digest(f"query relevancy n_pix={n_pix}", relevancy(x, dec, cuda(pos), cuda(neg)))


def main():
    if not torch.cuda.is_available():
        raise SystemExit("dense_digest.py runs the library's kernels; no GPU found")
    video()
    autoencoder()
    query()


if __name__ == "__main__":
    main()
