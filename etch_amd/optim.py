"""GuardedAdam: torch.optim.Adam with the NaN guards of the reference's training step (train.py:111-125) inside the step, on the device
(csrc/train_step.hip: etch_guarded_adam_step) -- two launches whatever the number of parameter tensors, no host synchronisation."""
import numpy as np
import torch

from . import _lib
from . import ops


class GuardedAdam(torch.optim.Optimizer):
    """`GuardedAdam(params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8)`: Adam with weight_decay = 0, amsgrad = False, maximize = False (anything else
    raises) over fp32 contiguous parameters of one device.  `step()` does on the device what train.py:111-125 does with one reduction and one
    blocking read per parameter tensor:

      * a tensor whose `grad.sum()` would be NaN is stepped with a zero gradient (its moments decay, its step count advances), as
        `param.grad = zeros_like(param.grad)` followed by `optimizer.step()` does.  "Would be NaN" = the gradient holds a NaN, or holds both +inf
        and -inf.  A gradient with infinities of ONE sign sums to an infinity, is not flagged and reaches the moments: faithful to the reference;
      * a tensor with `grad is None` is skipped altogether (no moment update, no step count), as torch.optim.Adam skips it;
      * if the loss kernel's status word (`self.status[0]`, written by etch_amd.losses.train_losses(..., status=optimizer.status)) says the total
        loss is NaN, the step changes nothing -- parameters, moments and step counts stay bit for bit -- and a device counter of skipped steps
        advances.  This is the ONE deviation from the reference, which prints "Loss is NaN issue" and then calls `.backward()` on the float 0.0
        (an AttributeError): skipping the step is its evident intent.

    The step counts live on the device (one fp32 per tensor; bias corrections are computed from them in the kernel).  Gradient addresses change from
    step to step (`zero_grad(set_to_none=True)`): they go up through a ring of pinned buffers, asynchronously; step() waits only if the host is more
    than RING steps ahead of the device.  `state_dict()` / `load_state_dict()` use torch.optim.Adam's layout, so a state saved by either loads into
    the other.  `step()` returns nothing; `report()` is the step's one readback.

    Accumulated and data-parallel steps: `accumulate(scale, first, losses)` packs each contribution's `.grad`s, scaled, into one flat buffer
    (`flat_gradients()`), the caller SUM-reduces that buffer over the ranks, and `step()` then takes its gradients from it: the guards above run on
    the combined gradient, and a NaN total in ANY contribution skips the step.  With one contribution and scale 1 the result is bit for bit the
    step from `.grad`."""

    RING = 4

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False):
        if weight_decay != 0 or amsgrad or maximize:
            raise ValueError("GuardedAdam supports weight_decay=0, amsgrad=False, maximize=False only")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"invalid lr / eps / betas: {lr}, {eps}, {betas}")
        # torch.optim.Adam's own param_groups keys, so the two state dicts are interchangeable
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False,
                        fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        self._groups = None
        self._status = None         # int32 (1): the loss kernel's status word
        self._counters = None       # int32 (4): tensors stepped with a zeroed gradient, skipped steps, bad-label flag (all cumulative), spare
        self._flat = None           # (fp32 buffer, layout) of flat_gradients()
        self._flat_losses = None
        self._flat_pending = False  # accumulate() since the last step(): the step reads the flat buffer

    # ---- tables
    def _check(self, p):
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.data_ptr() % 4:
            raise ValueError("GuardedAdam: parameters must be contiguous fp32 tensors on the GPU")

    def _device_tensors(self, device):
        if self._status is None:
            self._status = torch.zeros((1,), dtype=torch.int32, device=device)
            self._counters = torch.zeros((4,), dtype=torch.int32, device=device)

    @property
    def status(self):
        """The int32 device word that etch_amd.losses.train_losses(..., status=...) writes and step() obeys (None: no parameters)."""
        self._tables()
        return self._status

    @property
    def counters(self):
        self._tables()
        return self._counters

    def _build(self, group):
        """The static tables of one param group: chunk table, sizes, the device step counts and the pinned ring of the gradient addresses."""
        params = [p for p in group["params"] if p.numel() > 0]
        for p in params:
            self._check(p)
        dev = params[0].device
        if any(p.device != dev for p in params):
            raise ValueError("GuardedAdam: all parameters on one device")
        self._device_tensors(dev)
        chunk = ops.guarded_adam_chunk()
        T = len(params)
        numel = np.array([p.numel() for p in params], np.int64)
        nchunks = (numel + chunk - 1) // chunk
        first = np.zeros(T + 1, np.int64)
        np.cumsum(nchunks, out=first[1:])
        C = int(first[-1])
        if C >= 2 ** 31:
            raise ValueError("GuardedAdam: too many parameters for one group")
        g = {"params": params, "T": T, "C": C, "dev": dev,
             "chunk_tensor": torch.from_numpy(np.repeat(np.arange(T, dtype=np.int32), nchunks)).to(dev),
             "first_chunk": torch.from_numpy(first.astype(np.int32)).to(dev), "numel": torch.from_numpy(numel).to(dev),
             "steps": torch.zeros((T,), dtype=torch.float32, device=dev), "chunkflags": torch.zeros((C,), dtype=torch.int32, device=dev),
             "pmv_host": np.zeros((3, T), np.uint64), "pmv": torch.zeros((3, T), dtype=torch.int64, device=dev), "dirty": True,
             "ring": [torch.zeros((T,), dtype=torch.int64).pin_memory() for _ in range(self.RING)], "events": [None] * self.RING,
             "gdev": torch.zeros((T,), dtype=torch.int64, device=dev), "keep": None,
             "pptr": [-1] * T,          # the parameter address the tables hold; -1 = no state yet
             "numel_np": numel, "uploads": 0}
        g["ring_np"] = [r.numpy() for r in g["ring"]]
        # state that exists already (load_state_dict before the first step)
        for i, p in enumerate(params):
            st = self.state.get(p)
            if st:
                self._adopt(g, i, p, st)
        return g

    def _adopt(self, g, i, p, st):
        """Take a torch.optim.Adam-layout state entry over: moments contiguous fp32 on the device, the step count into the device array (of which
        state['step'] becomes a view)."""
        for k in ("exp_avg", "exp_avg_sq"):
            st[k] = st[k].to(device=p.device, dtype=torch.float32).contiguous()
            if st[k].numel() != p.numel():          # the kernel walks the moments by the parameter's size
                raise ValueError(f"GuardedAdam: state `{k}` has {st[k].numel()} elements for a parameter of {p.numel()}")
        view, step = g["steps"][i], st.get("step")
        if step is not None and not (torch.is_tensor(step) and step.is_cuda and step.data_ptr() == view.data_ptr()):
            view.fill_(float(step))          # a loaded state (reads a device step count back: never inside an ordinary step)
        st["step"] = view
        g["pmv_host"][:, i] = (p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr())
        g["pptr"][i] = p.data_ptr()
        g["dirty"] = True

    def _tables(self):
        if self._groups is None:
            self._flat, self._flat_pending = None, False          # the flat layout follows the tables
            self._groups = [self._build(group) if any(p.numel() for p in group["params"]) else None for group in self.param_groups]
        return self._groups

    # ---- the step
    def _gather(self, g):
        """The addresses of the group's current `.grad`s (0 = None), creating Adam state for a tensor that sees its first gradient."""
        ptrs, keep, pptr, f32 = [], [], g["pptr"], torch.float32
        for i, p in enumerate(g["params"]):
            grad = p.grad
            if grad is None:
                ptrs.append(0)
                continue
            if grad.dtype is not f32 or grad.device != p.device or grad.is_sparse:
                raise ValueError("GuardedAdam: gradients must be dense fp32 tensors on the parameters' device")
            if not grad.is_contiguous():
                grad = grad.contiguous()
                keep.append(grad)
            if pptr[i] != p.data_ptr():              # no state yet (torch.optim.Adam's lazy state: made at the first step that sees a gradient), or moved
                self._check(p)
                st = self.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                self._adopt(g, i, p, st)
            ptrs.append(grad.data_ptr())
        g["keep"] = keep
        return ptrs

    def _upload(self, g, ptrs):
        """An address table to the device through the pinned ring, asynchronously (and the parameter / moment table if it changed)."""
        slot = g["uploads"] % self.RING
        g["uploads"] += 1
        if g["events"][slot] is not None:
            g["events"][slot].synchronize()          # the copy of RING uploads ago: long done unless the host runs that far ahead
        g["ring_np"][slot][:] = ptrs
        if g["dirty"]:
            g["pmv"].copy_(torch.from_numpy(g["pmv_host"].view(np.int64)))
            g["dirty"] = False
            # what a step writes through this table (which tensors it really steps is known on the device only); state["step"] are views of g["steps"]
            states = [st for st in map(self.state.get, g["params"]) if st]
            g["written"] = g["params"] + [st[k] for st in states for k in ("exp_avg", "exp_avg_sq")] + [g["steps"], self._counters]
        g["gdev"].copy_(g["ring"][slot], non_blocking=True)
        ev = g["events"][slot] or torch.cuda.Event()
        ev.record()
        g["events"][slot] = ev

    @torch.no_grad()
    def step(self, closure=None):
        """One Adam step from the `.grad`s -- or, if accumulate() was called since the last step, from the flat buffer: the tail is unpacked first (the
        status word and `flat_losses`), and a tensor is stepped iff one of the local contributions held a gradient for it."""
        if closure is not None:
            raise ValueError("GuardedAdam.step takes no closure: a closure's loss would have to be read back")
        from_flat = self._flat_pending
        if from_flat:
            flat, layout = self.flat_gradients()
            ops.grad_unpack_tail(flat[layout["tail"]:], self._flat_losses, self._status)
        for group, g in zip(self.param_groups, self._tables()):
            if g is None:
                continue
            if from_flat:
                ptrs = np.where(g["has_grad"], flat.data_ptr() + 4 * g["off_np"], 0)
            else:
                ptrs = self._gather(g)
            self._upload(g, ptrs)
            lr, betas, eps = group["lr"], group["betas"], group["eps"]
            if group.get("weight_decay", 0) != 0 or group.get("amsgrad") or group.get("maximize"):
                raise ValueError("GuardedAdam supports weight_decay=0, amsgrad=False, maximize=False only")
            ops.guarded_adam_step(g["T"], g["C"], g["chunk_tensor"], g["first_chunk"], g["numel"], g["pmv"], g["gdev"], self._status, g["steps"],
                                  g["chunkflags"], float(lr), (float(betas[0]), float(betas[1])), float(eps), self._counters)
            _lib.wrote(*g["written"])
        self._flat_pending = False

    # ---- gradients through a flat buffer (accumulated and data-parallel steps)
    def flat_gradients(self):
        """(flat, layout): the fp32 device buffer accumulate() packs into, allocated at the first call, and its static layout -- {"params": the
        tensors, "offsets" / "numel": int64 arrays (tensor k at flat[offsets[k] : offsets[k] + numel[k]], every slot rounded up to 4 elements),
        "tail": the offset of the ops.grad_tail_floats() floats behind the slots (5 losses, NaN-total count, bad-label count, spare), "size"}.  The
        layout depends on the parameters alone, never on which gradients are None: it is the same on every rank."""
        if self._flat is None:
            groups = [g for g in self._tables() if g is not None]
            if not groups:
                raise ValueError("GuardedAdam.flat_gradients: no parameters")
            base, params, offs = 0, [], []
            for g in groups:
                slots = (g["numel_np"] + 3) // 4 * 4
                g["off_np"] = base + np.cumsum(slots) - slots
                g["off"] = torch.from_numpy(g["off_np"]).to(g["dev"])
                g["has_grad"] = np.zeros(g["T"], bool)
                base += int(slots.sum())
                params += g["params"]
                offs.append(g["off_np"])
            layout = {"params": params, "offsets": np.concatenate(offs), "numel": np.concatenate([g["numel_np"] for g in groups]), "tail": base,
                      "size": base + ops.grad_tail_floats()}
            self._flat = (torch.zeros((layout["size"],), dtype=torch.float32, device=groups[0]["dev"]), layout)
            self._flat_losses = torch.zeros((5,), dtype=torch.float32, device=groups[0]["dev"])
        return self._flat

    @property
    def flat_losses(self):
        """(5,) device tensor: the tail's losses as the last step from the flat buffer unpacked them (the sum over contributions of loss * scale)."""
        self.flat_gradients()
        return self._flat_losses

    @torch.no_grad()
    def accumulate(self, scale, first, losses=None):
        """Pack the current `.grad`s times `scale` into the flat buffer (csrc/train_step.hip: etch_grad_pack, one launch per param group): written if
        `first`, added otherwise; a None gradient contributes zeros.  The tail takes `losses` (the (5,) tensor of etch_amd.losses.train_losses, or
        None) times `scale` and the status word's bits.  The next step() reads the flat buffer -- reduce it over the ranks in between.

        Which tensors that step updates is decided per rank (a tensor is skipped iff its gradient was None in every LOCAL contribution): a model
        whose set of tensors with a gradient differs between ranks would step a tensor on one rank and not on another, and the replicas would
        drift apart unnoticed.  The set must be the same on every rank, as it is when every rank runs the same heads (`--pred_items`)."""
        flat, layout = self.flat_gradients()
        tail = layout["tail"]
        for g in self._tables():
            if g is None:
                continue
            ptrs = np.asarray(self._gather(g), np.int64)
            g["has_grad"] = (ptrs != 0) if first else (g["has_grad"] | (ptrs != 0))
            self._upload(g, ptrs)
            ops.grad_pack(g["T"], g["C"], g["chunk_tensor"], g["first_chunk"], g["numel"], g["gdev"], g["off"], flat, float(scale), 0 if first else 1,
                          losses if tail >= 0 else None, self._status if tail >= 0 else None, tail, layout=(g["off_np"], g["numel_np"]))
            tail = -1                                 # one tail per contribution: the first group's launch carries it
        self._flat_pending = True

    def report(self, losses=None):
        """The step's single readback: {"losses": the (5,) tensor the trainer hands over as a list (direction, magnitude, confidence, part label,
        total) or None, "tensors_zeroed", "skipped_steps" (both cumulative since construction), "bad_label" (a label outside [0, M) was seen)}."""
        if self.counters is None:
            return {"losses": None if losses is None else losses.tolist(), "tensors_zeroed": 0, "skipped_steps": 0, "bad_label": False}
        if losses is None:
            c = self.counters.tolist()
            vals = None
        else:
            both = torch.cat([losses.detach().reshape(-1).to(torch.float64), self.counters.to(torch.float64)]).tolist()
            vals, c = both[:-4], [int(x) for x in both[-4:]]
        return {"losses": vals, "tensors_zeroed": c[0], "skipped_steps": c[1], "bad_label": bool(c[2])}

    # ---- torch.optim.Adam's state layout
    def state_dict(self):
        sd = super().state_dict()
        # Adam's default layout keeps `step` as a 0-dim fp32 CPU tensor (the inner dicts are the live state's own: copied, not edited)
        sd["state"] = {k: {n: (v.detach().to("cpu", torch.float32).clone() if n == "step" else v) for n, v in st.items()} for k, st in sd["state"].items()}
        return sd

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._groups = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            if group.get("weight_decay", 0) != 0 or group.get("amsgrad") or group.get("maximize"):
                raise ValueError("GuardedAdam supports weight_decay=0, amsgrad=False, maximize=False only")
        self._groups = None          # rebuilt (and the loaded state adopted) at the next step
