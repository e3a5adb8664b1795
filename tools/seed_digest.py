"""SHA-256 of every output of the three LightGCN loss stages, for a bitwise
comparison of two builds of the library (MIREC_LIB selects the build):

    python tools/seed_digest.py > digest.txt
    MIREC_LIB=/path/to/other/libmirec.so python tools/seed_digest.py > other.txt

For fixed seeds it calls forward, loss, seed and reset of bpr.hip, ssm.hip and
ssm_shared.hip through the C ABI at D in (4, 64, 256), each loss with a key
count on either side of the sort threshold (8 192 pairs: the small sort up to
it, the radix sort above): BPR B = 2730 / 2731 (8 190 / 8 193 keys), sampled
softmax B = 257 with K = 29 / 33 (7 967 / 8 995), shared negatives B = 4000
with M = 100 / 257 (8 100 / 8 257).  User 1 and item 2 are planted HOT times
in every batch, so their runs are longer than 2 LPR + 1 = 129 entries at
every width.  One line per buffer: case, buffer, digest.  Every buffer is
allocated zeroed and hashed whole, the rows a kernel leaves alone included;
slot is hashed after the seed call and again after the reset.
"""
from __future__ import annotations

import ctypes
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from furusato_recommend_amd import _lib  # noqa: E402

NU, MI = 500, 3000
NN = NU + MI
HOT = 200
DECAY, LAYERS = 1e-4, 3
DEV = "cuda"


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def ok(rc, what):
    if rc != _lib.MIREC_OK:
        sys.exit(f"seed_digest: {what} returned {rc}")


def ids(gen, n, high, hot):
    v = torch.randint(0, high, (n,), generator=gen, dtype=torch.int32)
    v[:min(HOT, n)] = hot
    return v.to(DEV)


def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=DEV)


def finish(name, lib, st, n, query, seed_call, bufs):
    """Workspace, seed call, digests, reset; ``bufs`` = the forward's outputs."""
    nb = ctypes.c_size_t(0)
    ok(query(ctypes.byref(nb)), name + " workspace")
    ws = z(nb.value, dtype=torch.uint8)
    slot = torch.full((NN,), -1, dtype=torch.int32, device=DEV)
    ks = z(n, dtype=torch.int32)
    ok(seed_call(slot, ks, ws, nb.value), name + " seed")
    torch.cuda.synchronize()
    bufs.update(keys_sorted=ks, slot=slot)
    for k, v in bufs.items():
        print(name, k, sha(v))
    print(name, "ws_bytes", nb.value)
    ok(lib.mirec_bpr_seed_reset(slot.data_ptr(), ks.data_ptr(), n, st), name + " reset")
    torch.cuda.synchronize()
    print(name, "slot_after_reset", sha(slot), flush=True)


def main():
    lib, st = _lib.lib, _lib.stream_handle()
    for D in (4, 64, 256):
        gs = 0.25 if D == 64 else 1.0
        gen = torch.Generator().manual_seed(1000 + D)
        out = torch.randn(NN, D, generator=gen).to(DEV)
        emb = (0.1 * torch.randn(NN, D, generator=gen)).to(DEV)
        o, e = out.data_ptr(), emb.data_ptr()
        for B in (2730, 2731):
            n = 3 * B
            u, p, ng = ids(gen, B, NU, 1), ids(gen, B, MI, 2), ids(gen, B, MI, 3)
            coef, sp, reg, loss = z(B), z(B), z(B), z(1)
            keys, vals = z(n, dtype=torch.int32), z(n, dtype=torch.int32)
            seed_p, seed_e = z(n, D), z(n, D)
            ok(lib.mirec_bpr_forward(o, e, NN, NU, D, B, u.data_ptr(), p.data_ptr(),
                                     ng.data_ptr(), gs, coef.data_ptr(), sp.data_ptr(),
                                     reg.data_ptr(), keys.data_ptr(), vals.data_ptr(), st),
               "bpr_forward")
            ok(lib.mirec_bpr_loss(sp.data_ptr(), reg.data_ptr(), B, DECAY, loss.data_ptr(), None,
                                  st), "bpr_loss")
            finish(f"bpr D={D} B={B}", lib, st, n,
                   lambda nb: lib.mirec_bpr_seed_workspace(B, NN, nb),
                   lambda slot, ks, ws, nb: lib.mirec_bpr_seed(
                       o, e, NN, NU, D, B, u.data_ptr(), p.data_ptr(), ng.data_ptr(),
                       coef.data_ptr(), keys.data_ptr(), vals.data_ptr(), DECAY, gs, LAYERS,
                       slot.data_ptr(), seed_p.data_ptr(), seed_e.data_ptr(), ks.data_ptr(),
                       ws.data_ptr(), nb, st),
                   dict(coef=coef, loss=loss, seed_p=seed_p, seed_e=seed_e))
        B = 257
        for K in (29, 33):
            n = (2 + K) * B
            u, p = ids(gen, B, NU, 1), ids(gen, B, MI, 2)
            ng = ids(gen, B * K, MI, 2)
            coef, cpos, terms, reg, loss = z(B * K), z(B), z(B), z(B), z(1)
            g_u = z(B, D)
            keys, vals = z(n, dtype=torch.int32), z(n, dtype=torch.int32)
            seed_p, seed_e = z(n, D), z(n, D)
            ok(lib.mirec_ssm_forward(o, e, NN, NU, D, B, K, u.data_ptr(), p.data_ptr(),
                                     ng.data_ptr(), 0.2, gs, coef.data_ptr(), cpos.data_ptr(),
                                     terms.data_ptr(), reg.data_ptr(), g_u.data_ptr(),
                                     keys.data_ptr(), vals.data_ptr(), st), "ssm_forward")
            ok(lib.mirec_bpr_loss(terms.data_ptr(), reg.data_ptr(), B, DECAY, loss.data_ptr(),
                                  None, st), "bpr_loss")
            finish(f"ssm D={D} B={B} K={K}", lib, st, n,
                   lambda nb: lib.mirec_ssm_seed_workspace(B, K, NN, nb),
                   lambda slot, ks, ws, nb: lib.mirec_ssm_seed(
                       o, e, NN, NU, D, B, K, u.data_ptr(), coef.data_ptr(), cpos.data_ptr(),
                       g_u.data_ptr(), keys.data_ptr(), vals.data_ptr(), DECAY, gs, LAYERS,
                       slot.data_ptr(), seed_p.data_ptr(), seed_e.data_ptr(), ks.data_ptr(),
                       ws.data_ptr(), nb, st),
                   dict(coef=coef, coef_pos=cpos, g_u=g_u, loss=loss, seed_p=seed_p,
                        seed_e=seed_e))
        B = 4000
        for M in (100, 257):
            n = 2 * B + M
            u, p, sh = ids(gen, B, NU, 1), ids(gen, B, MI, 2), ids(gen, M, MI, 2)
            mask = (torch.rand(B * M, generator=gen) < 0.1).to(torch.uint8).to(DEV)
            coef, cpos, terms, reg, regs, loss = z(B * M), z(B), z(B), z(B), z(M), z(1)
            g = z(B + M, D)
            keys, vals = z(n, dtype=torch.int32), z(n, dtype=torch.int32)
            seed_p, seed_e = z(n, D), z(n, D)
            ok(lib.mirec_ssm_shared_forward(o, e, NN, NU, D, B, M, u.data_ptr(), p.data_ptr(),
                                            sh.data_ptr(), mask.data_ptr(), 0.2, gs,
                                            coef.data_ptr(), cpos.data_ptr(), terms.data_ptr(),
                                            reg.data_ptr(), regs.data_ptr(), g.data_ptr(),
                                            keys.data_ptr(), vals.data_ptr(), st),
               "ssm_shared_forward")
            ok(lib.mirec_ssm_shared_loss(terms.data_ptr(), reg.data_ptr(), regs.data_ptr(), B, M,
                                         DECAY, loss.data_ptr(), None, st), "ssm_shared_loss")
            finish(f"shared D={D} B={B} M={M}", lib, st, n,
                   lambda nb: lib.mirec_ssm_shared_seed_workspace(B, M, NN, nb),
                   lambda slot, ks, ws, nb: lib.mirec_ssm_shared_seed(
                       o, e, NN, NU, D, B, M, u.data_ptr(), cpos.data_ptr(), g.data_ptr(),
                       keys.data_ptr(), vals.data_ptr(), DECAY, gs, LAYERS, slot.data_ptr(),
                       seed_p.data_ptr(), seed_e.data_ptr(), ks.data_ptr(), ws.data_ptr(), nb,
                       st),
                   dict(coef=coef, coef_pos=cpos, g=g, loss=loss, seed_p=seed_p, seed_e=seed_e))


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("seed_digest: needs a HIP device")
    main()
