"""The argument checks that every BN op of bindings.cpp shares (bn_shape, check_same, check_channel_bufs,
check_ws): bn_act_backward and bn_relu_pool_backward used to hand mean / invstd / dgamma / dbeta, dx and ws
to the kernels unchecked.  A wrong buffer must be refused on the host, before any launch: RuntimeError, and no
tensor of the call is touched.  bn_act_forward takes the same mistakes in its own arguments of the same role
(save_mean for mean, scale for dgamma, y for dx)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, C, H, W = 2, 8, 4, 4
POOL = (3, 2, 1)                      # 4 x 4 -> 2 x 2
CL = torch.channels_last
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
OPS = ["bn_act_backward", "bn_relu_pool_backward", "bn_act_forward"]
# the argument of each op in the role the case names
ROLE = {
    "bn_act_backward": dict(mean="mean", dgamma="dgamma", dx="dx"),
    "bn_relu_pool_backward": dict(mean="mean", dgamma="dgamma", dx="dx"),
    "bn_act_forward": dict(mean="save_mean", dgamma="scale", dx="y"),
}


def _act(n, c, h, w, dtype, fill):
    return torch.full((n, c, h, w), fill, dtype=dtype, device="cuda").contiguous(memory_format=CL)


def _chan(c, fill):
    return torch.full((c,), fill, device="cuda")


def valid_args(op, dtype, c=C):
    """A valid call of ``op`` on [N, c, H, W]; every output is filled with a sentinel."""
    ops = torch.ops.gksgd
    eb = 2 if dtype == torch.bfloat16 else 4
    M = N * H * W
    # sized at a channel count both dtypes take (c itself may be one that bf16 does not)
    ws = torch.full((int(ops.bn_workspace_floats(M, 8, eb)) * max(1, c // 8),), 7.0, device="cuda")
    x = (torch.arange(N * c * H * W, device="cuda") % 7 - 3).to(dtype).view(N, c, H, W).contiguous(memory_format=CL)
    if op == "bn_act_forward":
        return dict(x=x, res=None, y=_act(N, c, H, W, dtype, 7.0),
                    mask=torch.full((M * c // (16 // eb),), 77, dtype=torch.uint8, device="cuda"),
                    w=_chan(c, 1.5), b=_chan(c, 0.25), run_mean=_chan(c, 0.0), run_var=_chan(c, 1.0),
                    save_mean=_chan(c, 7.0), save_invstd=_chan(c, 7.0), scale=_chan(c, 7.0), shift=_chan(c, 7.0),
                    ws=ws, eps=1e-5, momentum=0.1, relu=True)
    bwd = dict(x=x, dx=_act(N, c, H, W, dtype, 7.0), w=_chan(c, 1.5), mean=_chan(c, 0.0), invstd=_chan(c, 1.0),
               dgamma=_chan(c, 7.0), dbeta=_chan(c, 7.0), ws=ws)
    if op == "bn_act_backward":
        return dict(bwd, dy=_act(N, c, H, W, dtype, 0.5), dres=None, relu=True,
                    mask=torch.full((M * c // (16 // eb),), 0x55, dtype=torch.uint8, device="cuda"))
    k, s, p = POOL
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return dict(bwd, dy=_act(N, c, OH, OW, dtype, 0.5), k=k, s=s, p=p,
                amax=torch.full((N * c * OH * OW,), 4, dtype=torch.uint8, device="cuda"))


def break_args(op, dtype, case):
    role = ROLE[op]
    if case == "C=4":
        return valid_args(op, dtype, c=4)
    a = valid_args(op, dtype)
    if case == "fp16 mean":
        a[role["mean"]] = a[role["mean"]].half()
    elif case == "dgamma of C-1":
        a[role["dgamma"]] = _chan(C - 1, 7.0)
    elif case == "dx of another numel":
        a[role["dx"]] = _act(N - 1, C, H, W, dtype, 7.0)
    elif case == "CPU ws":
        a["ws"] = a["ws"].cpu()
    else:
        raise KeyError(case)
    return a


@DTYPES
@pytest.mark.parametrize("op", OPS)
def test_valid_call_runs(cuda, op, dtype):
    """The call the cases below spoil is itself accepted, and writes its outputs."""
    a = valid_args(op, dtype)
    getattr(torch.ops.gksgd, op)(**a)
    torch.cuda.synchronize()
    out = a[ROLE[op]["dx"]]
    assert not torch.equal(out, torch.full_like(out, 7.0))


# C = 4 is bf16's case: fp32 takes it (one 16-byte vector of channels)
CASES = [(case, dt) for case in ("fp16 mean", "dgamma of C-1", "dx of another numel", "CPU ws")
         for dt in (torch.bfloat16, torch.float32)] + [("C=4", torch.bfloat16)]


@pytest.mark.parametrize("case,dtype", CASES, ids=["%s-%s" % (c, str(d)[6:]) for c, d in CASES])
@pytest.mark.parametrize("op", OPS)
def test_bad_argument_refused(cuda, op, case, dtype):
    a = break_args(op, dtype, case)
    before = {k: v.clone() for k, v in a.items() if torch.is_tensor(v)}
    with pytest.raises(RuntimeError):
        getattr(torch.ops.gksgd, op)(**a)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(a[k], v), k
