"""Cases of the compact-record tests: ``(n, k_cap, ranks)``, per rank (ascending indices, fp32 values, header sent).
Reference: every rank's values rounded to bf16 by torch and scattered into a dense fp32 vector; the P vectors
added in rank order, one scale.  All comparisons are bit for bit."""
import torch

from gaussiank_sgd_amd import ops

SEG = 65536
CASES = ["one_segment", "boundary", "empty_middle", "empty_first", "empty_last", "sent_0", "sent_1",
         "full_odd_k_cap", "sent_over_k_cap", "long_run", "big_window", "p1", "p3_all_shared", "p17_all_shared",
         "p17_none_shared", "special_values"]


def _case(name):
    gen = torch.Generator().manual_seed(CASES.index(name))
    pick = lambda lo, hi, count: torch.sort(torch.randperm(hi - lo, generator=gen)[:count] + lo).values  # noqa: E731
    k_cap, sent, n, val = None, {}, 3 * SEG, None
    if name == "one_segment":
        n, idx = 64, [pick(0, 64, 9), pick(0, 64, 12)]
    elif name == "boundary":        # entries on both sides of a segment boundary
        n, idx = SEG + 64, [torch.tensor([3, 65535, 65536, 65570]), torch.tensor([65535, 65536])]
    elif name == "empty_middle":
        idx = [torch.cat((pick(0, SEG, 20), pick(2 * SEG, 3 * SEG, 20))) for _ in range(3)]
    elif name == "empty_first":
        idx = [pick(SEG, 3 * SEG, 30), pick(SEG + 100, 3 * SEG, 30)]
    elif name == "empty_last":
        idx = [pick(0, 2 * SEG, 30), pick(0, SEG, 30)]
    elif name == "sent_0":
        idx = [pick(0, n, 0), pick(0, n, 10)]
    elif name == "sent_1":
        idx = [torch.tensor([70000]), torch.tensor([70000])]
    elif name == "full_odd_k_cap":  # sent == k_cap, the last payload word half used
        idx, k_cap = [pick(0, n, 7), pick(0, n, 7)], 7
    elif name == "sent_over_k_cap":  # the header counts more than the record holds
        idx, k_cap, sent = [pick(0, n, 10), pick(0, n, 10)], 10, {0: 15}
    elif name == "long_run":        # more than 1,024 entries of one rank: several workgroups per rank
        idx = [pick(0, n, 1500), pick(0, n, 1300)]
        idx[1] = torch.unique(torch.cat((idx[0][:600], idx[1][600:])))
    elif name == "big_window":      # rank 1 holds more than the LDS window inside rank 0's key range
        base = pick(SEG, SEG + 6000, 3000)
        idx = [torch.cat((torch.tensor([5]), base[::75], torch.tensor([2 * SEG + 9]))), base]
    elif name == "special_values":
        # +-0, fp32 denormals, a tie, a value rounding up into the next binade, one within half a bf16 ulp of FLT_MAX
        sv = torch.tensor([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x3fffffff, 0x7f7fffff, 0x00008000,
                           0xbf80c000]).to(torch.int32).view(torch.float32)
        idx, val = [pick(0, n, sv.numel())] * 2, [sv, sv.flip(0).contiguous()]
    elif name == "p17_none_shared":  # more ranks than are staged in LDS
        idx = [pick(0, n // 17, 30) * 17 + q for q in range(17)]
    else:                            # p1, p3_all_shared, p17_all_shared
        idx = [pick(0, n, 40)] * int(name[1:].split("_")[0])
    k_cap = k_cap or max(i.numel() for i in idx) + 3
    val = val or [torch.randn(i.numel(), generator=gen) for i in idx]
    return n, k_cap, [(i, v, sent.get(q, i.numel())) for q, (i, v) in enumerate(zip(idx, val))]


def packed(name, device):
    """(n, k_cap, ranks, gathered compact records) from ops.pack_records16_, its own contract checked per rank."""
    n, k_cap, ranks = _case(name)
    words, nseg, half = ops.record16_words(n, k_cap), (n + SEG - 1) // SEG, (k_cap + 1) // 2
    gathered = torch.zeros(len(ranks) * words, dtype=torch.int32, device=device)
    gen = torch.Generator().manual_seed(1)
    for q, (idx, val, sent) in enumerate(ranks):
        m = idx.numel()
        rec = torch.zeros(ops.REC_HDR + 2 * k_cap, dtype=torch.int32)
        rec[0], rec[1] = sent, sent
        rec[ops.REC_HDR:ops.REC_HDR + m] = idx.to(torch.int32)
        rec[ops.REC_HDR + k_cap:ops.REC_HDR + k_cap + m] = val.view(torch.int32)
        r0 = torch.randn(n, generator=gen)
        r0[idx] = 0.0                                   # the selection cleared the sent slots
        rec_d, r_d = rec.clone().to(device), r0.clone().to(device)
        ops.pack_records16_(rec_d, k_cap, r_d, gathered[q * words:(q + 1) * words])
        rounded = val.to(torch.bfloat16).float()
        r0[idx] = val - rounded                         # the residue at the sent slots, nothing else touched
        assert torch.equal(r_d.cpu().view(torch.int32), r0.view(torch.int32)), "residual, rank %d" % q
        rec[ops.REC_HDR + k_cap:ops.REC_HDR + k_cap + m] = rounded.view(torch.int32)
        assert torch.equal(rec_d.cpu(), rec), "the full record keeps header and indices and gets the rounded values"
        c = gathered[q * words:(q + 1) * words].cpu()      # the layout, word for word
        assert c[:ops.REC_HDR].tolist() == rec[:ops.REC_HDR].tolist()
        assert c[ops.REC_HDR:ops.REC_HDR + nseg + 1].tolist() == [int((idx >> 16 < s).sum()) for s in range(nseg + 1)]
        pay = c[ops.REC_HDR + nseg + 1:].to(torch.int64) & 0xFFFFFFFF
        halves = torch.stack((pay & 0xFFFF, pay >> 16), 1).view(2, 2 * half)
        bf = (rounded.view(torch.int32).to(torch.int64) >> 16) & 0xFFFF
        assert halves[:, :m].tolist() == [(idx & 0xFFFF).tolist(), bf.tolist()] and not halves[:, m:].any()
    return n, k_cap, ranks, gathered


def check_reduce(name, device, apply):
    n, k_cap, ranks, gathered = packed(name, device)
    P = len(ranks)
    total, seen = torch.zeros(n), torch.zeros(n, dtype=torch.bool)
    for idx, val, _ in ranks:
        dense = torch.zeros(n)
        dense[idx] = val.to(torch.bfloat16).float()
        total = total + dense
        seen[idx] = True
    scale = torch.tensor(1.0 / P, dtype=torch.float32)
    dst0 = torch.randn(n, generator=torch.Generator().manual_seed(2))
    dst = dst0.clone().to(device)
    if not apply:
        ops.reduce_records16_(dst, gathered, P, k_cap, 1.0 / P)
        want = torch.where(seen, dst0 + total * scale, dst0)
        assert torch.equal(dst.cpu().view(torch.int32), want.view(torch.int32))
        return
    shadow0 = torch.full((n,), 7.0, dtype=torch.bfloat16)
    shadow = shadow0.clone().to(device)
    ops.reduce_records16_(dst, gathered, P, k_cap, 1.0 / P, lr=0.1, lr_mult=torch.tensor([0.5], device=device),
                          w_bf16=shadow)
    lr = torch.tensor(0.1, dtype=torch.float32) * torch.tensor(0.5, dtype=torch.float32)
    want = torch.where(seen, dst0 - lr * (total * scale), dst0)
    assert torch.equal(dst.cpu().view(torch.int32), want.view(torch.int32))
    assert torch.equal(shadow.cpu().view(torch.int16), torch.where(seen, want.to(torch.bfloat16), shadow0).view(torch.int16))
