"""Training-step timing of BASELINE.json configs[2]'s per-GPU share (GPU box): HigherHRNet-W32, batch B @ 512x512,
forward (train-mode BN) + AE loss + backward + Adam.  python tools/train_bench.py [B] [steps] [--precision bf16|fp16] [--rounds N]
[--optimizer torch|hip] [--max-grad-norm X] [--clip auto|torch]
--precision fp16: fp16 activations and the reference's GradScaler sequence (scale(loss).backward(), scaler.step, scaler.update);
bf16 (default): no scaler.  --optimizer hip: the one-launch Adam of pytorch-human-pose_amd/optim.py (and its GradScaler in fp16) instead
of torch.optim.Adam (default; HH_FUSED_ADAM=1 selects torch's fused kernels there).  Each line also gives the HOST time of the optimizer
call per step (the clip, where there is one, and scaler.step or opt.step: asynchronous, so this is launch and bookkeeping time, not kernel time).
--max-grad-norm X: clip the gradients to global norm X between the backward (fp16: scaler.unscale_) and the step, with
pkg.optim.clip_grad_norm_ (--clip auto: the device table's launches for --optimizer hip, torch's function for torch) or with
torch.nn.utils.clip_grad_norm_ whatever the optimizer (--clip torch).  The line then ends with the last step's norm.
--rounds N: N timed rounds of `steps` steps each, one line per round (their spread is the noise floor)."""
import argparse
import importlib, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
pkg = importlib.import_module("pytorch-human-pose_amd")
ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=32)
ap.add_argument("steps", nargs="?", type=int, default=5)
ap.add_argument("--precision", choices=("bf16", "fp16"), default="bf16")
ap.add_argument("--rounds", type=int, default=1)
ap.add_argument("--optimizer", choices=("torch", "hip"), default="torch")
ap.add_argument("--max-grad-norm", type=float, default=None)
ap.add_argument("--clip", choices=("auto", "torch"), default="auto")
args = ap.parse_args()
B, steps = args.B, args.steps
K, S = 17, 512
net = pkg.HigherHRNet(K, 32)
net.load_state_dict({k: torch.from_numpy(pkg.synth.synth_param(k, v.shape, 0)) for k, v in net.state_dict().items()})
net = net.cuda().train()
net.set_train_precision(args.precision)
hip = args.optimizer == "hip"
scaler = (pkg.optim.GradScaler if hip else torch.amp.GradScaler)("cuda") if args.precision == "fp16" else None
loss_fn = pkg.AEKeypointsLoss()
if hip:
    opt = pkg.optim.Adam(net.parameters(), lr=1e-4)
else:
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, **({"fused": True} if os.environ.get("HH_FUSED_ADAM") else {}))
opt_host = [0.0]
params = list(net.parameters())
grad_norm = [None]
if args.max_grad_norm is not None and hip and args.clip == "auto":
    opt.collect_grad_stats = True  # (as the modules do: the unscale launch leaves the statistics)
def clip():
    if args.clip == "torch":
        grad_norm[0] = torch.nn.utils.clip_grad_norm_(params, args.max_grad_norm)
    else:
        grad_norm[0] = pkg.optim.clip_grad_norm_(opt, args.max_grad_norm)
x = torch.from_numpy(pkg.synth.synth_images(B, S, S, 0)).cuda()
hms, masks, joints = pkg.synth.synth_train_targets(B, K, S, 10, seed=0)
hms = [torch.from_numpy(h).cuda() for h in hms]; masks = [torch.from_numpy(m).cuda() for m in masks]
def step():
    ph, pt = net(x)
    hl, push, pull = loss_fn.calculate_loss(ph, pt, hms, masks, joints)
    loss = hl[0] + hl[1] + push[0] + pull[0]
    opt.zero_grad(set_to_none=True)
    if scaler is None:
        loss.backward()
        t0 = time.perf_counter()
        if args.max_grad_norm is not None: clip()
        opt.step()
    else:
        scaler.scale(loss).backward()
        t0 = time.perf_counter()
        if args.max_grad_norm is not None:
            scaler.unscale_(opt); clip()
        scaler.step(opt)
    opt_host[0] += time.perf_counter() - t0
    if scaler is not None:
        scaler.update()
    return loss
for _ in range(2): l = step()
for _ in range(args.rounds):
    torch.cuda.synchronize(); t = time.perf_counter(); opt_host[0] = 0.0
    for _ in range(steps): l = step()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t) / steps
    print(f"train step {args.precision} optimizer={args.optimizer} B={B} @ {S}x{S}: {dt*1e3:.1f} ms/step  optimizer host {opt_host[0]/steps*1e3:.2f} ms/step  {B/dt:.1f} img/s  loss {l.item():.5f}  peak mem {torch.cuda.max_memory_allocated()/2**30:.1f} GiB"
          + (f"  loss scale {scaler.get_scale():.0f}" if scaler is not None else "")
          + (f"  max_grad_norm {args.max_grad_norm:g} ({args.clip}) grad_norm {grad_norm[0].item():.6g}" if grad_norm[0] is not None else ""), flush=True)
