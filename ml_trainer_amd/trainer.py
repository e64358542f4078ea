"""Trainer -- the training-lifecycle engine (reference ``src/trainer.py:22-311``).

Public contract kept exactly:
``Trainer(model, datasets=None, epochs=None, batch_size=None, is_parallel=False,
save_history=False, **config)`` with the same 11-key config whitelist and
defaults, ``fit()``, ``test(model, loader)``, ``save_model(dir)``,
``save_history_(dir)``, ``clear()``, ``validate_kwargs(...)``, the attributes
``train_loader``/``val_loader``/``history``/``train_losses``..., the log lines
and the ``model.pth`` / ``history.pkl`` artifacts. Added public methods named by
the north star: ``train_step(batch)`` and ``evaluate(loader=None)``.

Under that surface (MI355X-first):

* **fused step engine** -- for the reference LeNet on a GPU the whole training
  step (augmentation, fwd, CE, metrics, bwd, optimizer) runs natively: bf16 as
  TWO kernels per step (the per-sample chain ``lenet_ms``, then the batch
  reductions + optimizer update + next-step input prep ``lenet_mw``), fp32 as
  four, replayed as multi-step hipGraphs
  (``models/lenet_engine.py``): no per-step host syncs (fix B12), no H2D copies
  (HBM-resident dataset);
* **generic path** -- any ``nn.Module``: native fused optimizer over a flat
  parameter buffer, native flat-bucket DDP with backward-overlapped RCCL
  all-reduce, pinned-host prefetch on a copy stream, on-device loss/metric
  accumulation (one sync per epoch), optional bf16 autocast;
* fixes of the reference's defects: device bound before
  wrapping (B6), model never moved to CPU by checkpointing (B5), broken
  criteria instantiated (B7), only the selected scheduler constructed and
  ReduceLROnPlateau stepped on val loss (B8), ``set_epoch`` called (B11),
  ``test()`` under ``eval()``/``no_grad`` (B13), atomic rank-0 checkpoint +
  barrier (§5.3).
"""
from __future__ import annotations

import gc
import json
import math
import os
import random
import time
import warnings
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist
from torch import nn

from ml_trainer_amd.config import ALLOWED_KWARGS, CONFIG_DEFAULTS, TrainerOptions
from ml_trainer_amd.data.loader import DeviceDataset, DevicePrefetcher, Loader, device_dataset_spec
from ml_trainer_amd.ops import losses as L
from ml_trainer_amd.ops._ext import native_available
from ml_trainer_amd.ops.optim import FusedOptimizer, build_optimizer
from ml_trainer_amd.parallel import dist as mdist
from ml_trainer_amd.parallel.ddp import DistributedDataParallel
from ml_trainer_amd.parallel.zero import ZeroDataParallel
from ml_trainer_amd.parallel.sampler import ShardSampler
from ml_trainer_amd.utils import checkpoint as ckpt
from ml_trainer_amd.utils.flat import FlatParams
from ml_trainer_amd.utils.functions import custom_loss_function
from ml_trainer_amd.utils.logging import get_logger
from ml_trainer_amd.utils.profiling import StepTimer, range_ctx
from ml_trainer_amd.utils.watchdog import Watchdog

logger = get_logger("__name__")  # the reference names its logger with the literal string (src/trainer.py:19)


def _tqdm(iterable=None, total=None, disable=False, **kw):
    try:
        from tqdm import tqdm
        return tqdm(iterable, total=total, disable=disable, unit="batch", **kw)
    except ImportError:  # pragma: no cover
        class _N:
            def __init__(self, it):
                self.it = it

            def __iter__(self):
                return iter(self.it if self.it is not None else [])

            def update(self, n=1):
                pass

            def set_postfix(self, **k):
                pass

            def close(self):
                pass

            def __enter__(self):
                return self

            def __exit__(self, *a):
                return False
        return _N(iterable)


class _CustomLoss(nn.Module):
    """Wraps a plain loss function so ``.to(device)`` works (reference B7: 'custom' crashed)."""

    def __init__(self, fn: Callable):
        super().__init__()
        self.fn = fn

    def forward(self, output, target):
        return self.fn(output, target)


class Trainer:
    def __init__(self, model, datasets=None, epochs=None, batch_size=None, is_parallel=False, save_history=False,
                 options=None, **config):
        logger.info("Config inputs.", config=config)
        self.validate_kwargs(config, ALLOWED_KWARGS)
        self.opts = TrainerOptions.from_any(options)
        cfg = {k: (config[k] if k in config else v) for k, v in CONFIG_DEFAULTS.items()}
        self.config = cfg
        self.epochs = epochs
        self.scheduler_type = cfg["scheduler"]
        self.optimizer_type = cfg["optimizer"]
        self.momentum = cfg["momentum"]
        self.weight_decay = cfg["weight_decay"]
        self.lr = cfg["lr"]
        self.criterion_type = cfg["criterion"]
        self.metric = cfg["metric"]
        per_tensor = self.opts.no_decay_1d or str(self.optimizer_type or "").lower() == "lamb"
        if self.opts.zero_stage == 1 and per_tensor:
            raise ValueError("zero_stage=1 cannot be combined with optimizer 'lamb' or no_decay_1d: ZeRO-1 shards "
                             "cut tensors, and a per-tensor norm or decay over a sharded tensor needs a collective")
        self.pred_function_type = cfg["pred_function"]
        self.model_dir = cfg["model_dir"]
        backend = cfg["backend"]
        seed = cfg["seed"]
        self.seed = seed
        train_set = val_set = None
        if datasets:
            train_set, val_set = datasets
        torch.manual_seed(seed)
        self.model = model
        self.is_parallel = is_parallel
        self.save_history = save_history
        self.train_losses: List[float] = []
        self.val_losses: List[float] = []
        self.train_metrics: List[float] = []
        self.val_metrics: List[float] = []
        self.history: Dict[str, Any] = {}
        self.throughput: List[Dict[str, float]] = []
        logger.info("Loading the model.")
        self.world_size, self.rank = 1, 0
        train_sampler = None
        if self.is_parallel:
            if datasets:
                self.rank, self.world_size, self.dist_backend = mdist.init_distributed(
                    backend, timeout_s=self.opts.dist_timeout_s)
                train_sampler = ShardSampler(train_set, num_replicas=self.world_size, rank=self.rank)
                if not self.opts.per_device_batch:
                    # reference semantics: the global batch is split across ranks (src/trainer.py:62-64)
                    batch_size = max(batch_size // self.world_size, 1)
            else:
                logger.warning("Testing only available. No datasets in arguments.")
        elif not datasets:
            logger.warning("Testing only available. No datasets in arguments.")
        # B6 fix: bind LOCAL_RANK's GPU before the model is placed or wrapped
        self.device = mdist.bind_device(prefer_gpu=True)
        logger.info(f"Training on device: {self.device}.")
        self.batch_size = batch_size
        self.train_sampler = train_sampler
        if datasets:
            logger.info("Loading training and validation set.")
            logger.info("Preparing the data.")
            pin = self.opts.pin_memory and self.device.type == "cuda"
            self.train_loader = Loader(train_set, batch_size=batch_size, shuffle=train_sampler is None,
                                       sampler=train_sampler, num_workers=self.opts.num_workers, pin_memory=pin)
            self.val_loader = Loader(val_set, batch_size=batch_size, shuffle=True,
                                     num_workers=self.opts.num_workers, pin_memory=pin)
            logger.debug("Processes {}/{} ({:.0f}%) of train data".format(
                len(self.train_loader.sampler), len(self.train_loader.dataset),
                100.0 * len(self.train_loader.sampler) / max(len(self.train_loader.dataset), 1)))
            logger.debug("Processes {}/{} ({:.0f}%) of validation data".format(
                len(self.val_loader.sampler), len(self.val_loader.dataset),
                100.0 * len(self.val_loader.sampler) / max(len(self.val_loader.dataset), 1)))
        else:
            logger.warning("Testing only available. No datasets in arguments.")
        self.model = self.model.to(self.device)
        self._core = self.model
        self._zero = None
        if self.is_parallel and mdist.is_dist():
            if self.opts.zero_stage not in (0, 1):
                raise ValueError("zero_stage must be 0 or 1")
            ddp_cls = ZeroDataParallel if self.opts.zero_stage == 1 else DistributedDataParallel
            self.model = ddp_cls(self.model, bucket_cap_mb=self.opts.bucket_cap_mb,
                                 first_bucket_mb=self.opts.first_bucket_mb, mode=self.opts.ddp_mode)
            self.flat: Optional[FlatParams] = self.model.flat
            if self.opts.zero_stage == 1:
                self._zero = self.model
        else:
            has_params = any(p.requires_grad for p in self.model.parameters())
            self.flat = FlatParams(self.model.parameters()) if has_params else None
        criterion = self._get_criterion()
        self.criterion = criterion.to(self.device) if hasattr(criterion, "to") else criterion
        self.optimizer = self._get_optimizer()
        self.scheduler_options = {
            "CosineAnnealingWarmRestarts": lambda: torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(
                self.optimizer, T_0=5, eta_min=1e-7),
            "ReduceLROnPlateau": lambda: torch.optim.lr_scheduler.ReduceLROnPlateau(self.optimizer, "min",
                                                                                    min_lr=1e-7),
            "StepLR": lambda: torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=2),
        }
        self.scheduler = None
        if self.scheduler_type:
            self.scheduler = self.scheduler_options[self.scheduler_type]()  # unknown name -> KeyError (reference)
        self.pred_function = self._get_prediction_function()
        self.global_step = 0
        self.start_epoch = 1
        self._engine = None
        self._val_engine = None
        self._dev_train: Optional[DeviceDataset] = None
        self._dev_val: Optional[DeviceDataset] = None
        wd = self.opts.watchdog_s
        if wd is None:  # default: on for multi-rank jobs (a dead peer must not hang the others)
            wd = 600.0 if (self.is_parallel and mdist.world_size() > 1) else 0.0
        self._watchdog = Watchdog(wd) if wd > 0 else None
        if self.opts.resume:
            self._resume()

    # ------------------------------------------------------------------ factories
    def _get_prediction_function(self):
        if self.pred_function_type == "logsoftmax":
            return nn.LogSoftmax(dim=-1)
        if self.pred_function_type == "softmax":
            return nn.Softmax(dim=-1)
        return None

    def _get_optimizer(self):
        params = list(self._core.parameters())
        if not any(p.requires_grad for p in params):
            return None
        opt = build_optimizer(self.optimizer_type, params, lr=self.lr, momentum=self.momentum,
                              weight_decay=self.weight_decay,
                              flat=self._zero.shard if self._zero is not None else self.flat,
                              no_decay_1d=self.opts.no_decay_1d)
        if opt is None:
            raise ValueError(f"unknown optimizer {self.optimizer_type!r} (sgd|adam|adagrad|adamax|adamw|lamb)")
        return self._zero.attach_optimizer(opt) if self._zero is not None else opt

    def _get_criterion(self):
        c = self.criterion_type
        if c == "cross_entropy":
            return L.CrossEntropyLoss()
        if c == "neg-loss":
            return L.NLLLoss()
        if c == "l1":
            return L.L1Loss()
        if c == "l2":
            return L.MSELoss()
        if c == "custom":
            return _CustomLoss(custom_loss_function)
        if c == "mlm":  # masked-LM pre-training: the model's own head over its hidden states
            if not hasattr(self._core, "mlm_loss"):
                raise ValueError("criterion 'mlm' needs a model with an mlm_loss head (BertForMaskedLM)")
            return _CustomLoss(self._core.mlm_loss)
        if c == "clm":  # causal language model: the same head on next-token labels
            if not hasattr(self._core, "lm_loss"):
                raise ValueError("criterion 'clm' needs a model with an lm_loss head (BertLMHeadModel)")
            return _CustomLoss(self._core.lm_loss)
        if callable(c):
            return c if isinstance(c, nn.Module) else _CustomLoss(c)
        raise ValueError(f"unknown criterion {c!r} (cross_entropy|neg-loss|l1|l2|custom|mlm|clm or a callable)")

    def _average_gradients(self):
        """Manual gradient averaging (reference src/trainer.py:152-158): one flat all-reduce."""
        if isinstance(self.model, DistributedDataParallel):
            self.model.sync_gradients()
        elif mdist.is_dist() and self.flat is not None:
            dist.all_reduce(self.flat.grad)
            self.flat.grad.mul_(1.0 / mdist.world_size())

    # ------------------------------------------------------------------ metrics
    def _get_predictions(self, outputs):
        # argmax(softmax(x)) == argmax(x): skip the monotone prediction functions
        if self.pred_function_type in ("softmax", "logsoftmax") or self.pred_function is None:
            return torch.argmax(outputs, dim=-1)
        return torch.argmax(self.pred_function(outputs), dim=-1)

    def _evaluate(self, outputs, targets):
        """Per-batch metric as a device tensor (reference returns a host float: B12 fix)."""
        if self.metric == "mcrmse":
            return L.mcrmse(outputs, targets)
        if self.metric == "accuracy":
            if self.criterion_type in ("mlm", "clm"):  # masked- / next-token accuracy of the criterion call just made
                return self._core.last_mlm_accuracy
            return L.accuracy(outputs, targets)
        return None

    def _metric_outputs(self, outputs):
        """What ``_evaluate`` takes: the fp32 outputs (criterion 'mlm' / 'clm': the hidden states as they are,
        its metric comes from the head)."""
        return outputs.detach() if self.criterion_type in ("mlm", "clm") else outputs.detach().float()

    # ------------------------------------------------------------------ engine selection
    def _engine_eligible(self, for_eval: bool = False) -> bool:
        o = self.opts
        if o.use_engine is False or self.device.type != "cuda" or not native_available():
            self._warn_precision_ignored()
            return False
        from ml_trainer_amd.models.lenet import MLModel
        ok = (isinstance(self._core, MLModel) and self.criterion_type == "cross_entropy"
              and self.metric in ("accuracy", None) and self.pred_function_type in (None, "softmax", "logsoftmax")
              and isinstance(self.optimizer, FusedOptimizer) and len(self.optimizer.param_groups) == 1
              and not self.optimizer.per_tensor  # the engine's kernels embed the five element-wise rules
              and self.optimizer.flats[0] is self.flat and o.grad_accum_steps == 1 and o.grad_clip is None
              and o.amp is None)
        if not ok:
            if o.use_engine:
                raise RuntimeError("use_engine=True but the model/criterion/optimizer/options are not supported "
                                   "by the fused LeNet engine")
            self._warn_precision_ignored()
            return False
        loader = self.val_loader if for_eval else self.train_loader
        if o.device_data is False or device_dataset_spec(loader.dataset) is None:
            if o.use_engine:
                raise RuntimeError("use_engine=True needs a device-capable dataset (uint8 [N,32,32,3])")
            self._warn_precision_ignored()
            return False
        return True

    def _warn_precision_ignored(self) -> None:
        """precision='bf16' is the fused LeNet engine's step dtype; any other path trains in fp32."""
        if self.opts.precision == "bf16" and not getattr(self, "_prec_warned", False):
            self._prec_warned = True
            warnings.warn("precision='bf16' applies to the fused LeNet engine only, which is not used for this "
                          "run (model / criterion / optimizer / options / dataset): training runs in fp32; "
                          "use amp='bf16' for bf16 autocast on generic models")

    def _get_engine(self):
        from ml_trainer_amd.models.lenet_engine import LeNetStepEngine
        if self._engine is None:
            n_steps = len(self.train_loader)
            self._engine = LeNetStepEngine(self._core, self.flat, max_batch=self.batch_size,
                                           world_size=self.world_size, seed=self.seed,
                                           precision=self.opts.precision)
            self._engine.set_optimizer(self.optimizer,
                                       lr_table_len=n_steps if self.scheduler_type == "CosineAnnealingWarmRestarts"
                                       else 0)
            self._dev_train = DeviceDataset(self.train_loader.dataset, self.device)
            s = self._dev_train.spec
            n_idx = len(self.train_loader.sampler)
            self._engine.set_dataset(self._dev_train.data, self._dev_train.targets, self.batch_size,
                                     augment=True, pad=s["pad"], flip=s["flip"], mean=s["mean"], std=s["std"],
                                     perm_capacity=n_idx)
            self._engine.ctrl[0:1].fill_(self.global_step)
            eng = self._engine
            if mdist.is_dist():
                # line the ranks up after each built its device dataset (the first in-graph
                # collective of the step graphs then starts within a small skew on every rank)
                dist.barrier()
            if self._watchdog is not None and eng.comm is not None and eng.dp_transport == "rccl":
                self._watchdog.add_probe(eng.comm.async_error, eng.comm.abort)
            if self._watchdog is not None and eng.xgmi is not None and eng.dp_transport.startswith("xgmi"):
                x = eng.xgmi
                self._watchdog.add_probe(lambda: "xGMI all-reduce peer timeout" if x.error() else "")
        return self._engine

    def _get_val_engine(self):
        from ml_trainer_amd.models.lenet_engine import LeNetStepEngine
        if self._val_engine is None:
            self._val_engine = LeNetStepEngine(self._core, self.flat, max_batch=self.batch_size,
                                               world_size=1, seed=self.seed + 1)
            self._dev_val = DeviceDataset(self.val_loader.dataset, self.device)
            s = self._dev_val.spec
            self._val_engine.set_dataset(self._dev_val.data, self._dev_val.targets, self.batch_size, augment=True,
                                         pad=s["pad"], flip=s["flip"], mean=s["mean"], std=s["std"])
        return self._val_engine

    # ------------------------------------------------------------------ training
    def train_step(self, batch) -> torch.Tensor:
        """One optimisation step on ``batch=(inputs, targets)``; returns the detached loss (device)."""
        inputs, targets = batch
        inputs = inputs.to(self.device, non_blocking=True)
        targets = targets.to(self.device, non_blocking=True)
        self.model.train()
        if self.optimizer is not None:
            self.optimizer.zero_grad()
        loss, outputs = self._forward_backward(inputs, targets)
        self._optimizer_step()
        self._last_outputs = outputs.detach()
        return loss.detach()

    def _forward_backward(self, inputs, targets, sync: bool = True):
        ctx = torch.autocast(device_type=self.device.type, dtype=torch.bfloat16) if self.opts.amp == "bf16" \
            else _nullctx()
        if isinstance(self.model, DistributedDataParallel) and not sync:
            nosync = self.model.no_sync()
        else:
            nosync = _nullctx()
        with nosync:
            with ctx:
                outputs = self.model(inputs)
                loss = self.criterion(outputs, targets)
            scale = 1.0 / self.opts.grad_accum_steps
            (loss * scale if scale != 1.0 else loss).backward()
            if sync and isinstance(self.model, DistributedDataParallel):
                self.model.after_backward()
        return loss, outputs

    def _optimizer_step(self):
        if self.optimizer is None:
            return
        if self.opts.grad_clip is not None and self._zero is not None:
            self._zero.clip_grad_norm_(self.opts.grad_clip)
        elif self.opts.grad_clip is not None and self.flat is not None:
            from ml_trainer_amd.ops.optim import clip_grad_norm_flat
            clip_grad_norm_flat(self.flat, self.opts.grad_clip)
        self.optimizer.step()
        self.global_step += 1
        self._maybe_inject_fault()

    def _maybe_inject_fault(self):
        o = self.opts
        if o.fault_inject_step >= 0 and self.global_step == o.fault_inject_step and self.rank == o.fault_inject_rank:
            raise RuntimeError(f"injected fault at global step {self.global_step} on rank {self.rank}")

    def _cosine_lr_table(self, epoch: int, n: int) -> List[float]:
        """Per-step lrs of this epoch, produced by the real scheduler in the reference order
        (lr of step i is read before ``scheduler.step(epoch - 1 + i / n)``, src/trainer.py:188-190)."""
        lrs = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for i in range(n):
                lrs.append(float(self.optimizer.param_groups[0]["lr"]))
                self.scheduler.step(epoch - 1 + i / n)
        return lrs

    def _train_one_epoch(self, epoch: int):
        self.model.train()
        if self.train_sampler is not None:
            self.train_sampler.set_epoch(epoch)  # B11 fix
        n = len(self.train_loader)
        with StepTimer(self.device) as tm, range_ctx(f"train_epoch_{epoch}", self.opts.profile_ranges):
            if self._engine_eligible():
                loss, metric, samples = self._engine_train_epoch(epoch, n)
            else:
                loss, metric, samples = self._generic_train_epoch(epoch, n)
        dt = tm.wall_ms / 1e3
        if self.scheduler_type == "StepLR":
            self.scheduler.step()
        if self.opts.global_metrics and mdist.is_dist():
            loss, metric = self._global_mean(loss, metric)
        self.train_losses.append(loss)
        if self.metric:
            self.train_metrics.append(metric)
        rec = {"epoch": epoch, "train_time_s": dt, "steps": n, "samples_rank": samples,
               "samples_per_s_rank": samples / dt if dt > 0 else 0.0,
               "samples_per_s_node": samples * self.world_size / dt if dt > 0 else 0.0,
               "ms_per_step": dt / max(n, 1) * 1e3, "device_ms_per_step": tm.device_ms / max(n, 1)}
        self.throughput.append(rec)
        logger.info("train throughput", samples_per_s=round(rec["samples_per_s_node"], 1),
                    ms_per_step=round(rec["ms_per_step"], 4), epoch=epoch)

    def _engine_train_epoch(self, epoch: int, n: int):
        eng = self._get_engine()
        if self.train_sampler is not None:
            idx = torch.as_tensor(self.train_sampler.indices(), dtype=torch.int32)
        else:
            idx = torch.randperm(len(self.train_loader.dataset)).to(torch.int32)
        lrs = self._cosine_lr_table(epoch, n) if self.scheduler_type == "CosineAnnealingWarmRestarts" else None
        eng.start_epoch(idx, lrs)
        eng.reset_stats()
        B = self.batch_size
        full, last = divmod(idx.numel(), B)
        spg = max(1, self.opts.steps_per_graph)
        bar = _tqdm(total=n, disable=not (self.opts.progress and self.rank == 0))
        done = 0
        while done < full:
            k = min(spg, full - done)
            eng.train_steps(B, k, use_graph=self.opts.use_graph, steps_per_graph=spg)
            done += k
            bar.update(k)
            if self._watchdog:
                self._watchdog.beat()
        if last:
            eng.train_steps(last, 1, use_graph=self.opts.use_graph, steps_per_graph=1)
            bar.update(1)
        loss, acc = eng.read_stats(n)  # the ONE host sync of the epoch
        eng.check_transport()
        bar.set_postfix(loss=loss, metric=acc if self.metric else None)
        bar.close()
        self.global_step += n
        self.optimizer._steps[0] = self.global_step  # keep the optimizer's step count (checkpoints) in sync
        self._maybe_inject_fault()
        return loss, (acc if self.metric else None), idx.numel()

    def _device_batches(self, loader, train: bool):
        """Yield device batches: HBM-resident + GPU augmentation when possible, else pinned prefetch."""
        if (self.device.type == "cuda" and self.opts.device_data is not False and native_available()
                and device_dataset_spec(loader.dataset) is not None):
            from ml_trainer_amd.ops.augment import DeviceAugmentIterator
            dd = self._dev_train if train else self._dev_val
            if dd is None:
                dd = DeviceDataset(loader.dataset, self.device)
                if train:
                    self._dev_train = dd
                else:
                    self._dev_val = dd
            if train and self.train_sampler is not None:
                idx = torch.as_tensor(self.train_sampler.indices(), dtype=torch.int32)
            else:
                idx = torch.randperm(len(loader.dataset)).to(torch.int32)
            step0 = self.global_step if train else len(self.val_losses) * 1_000_003
            return DeviceAugmentIterator(dd, idx, self.batch_size, seed=self.seed + (0 if train else 1),
                                         step0=step0, advance_step=train)
        if self.device.type == "cuda":
            return DevicePrefetcher(loader, self.device, depth=self.opts.prefetch_depth)
        return loader

    def _generic_train_epoch(self, epoch: int, n: int):
        running_loss = torch.zeros((), dtype=torch.float64, device=self.device)
        running_metric = torch.zeros((), dtype=torch.float64, device=self.device)
        samples = 0
        acc_steps = max(1, self.opts.grad_accum_steps)
        it = self._device_batches(self.train_loader, train=True)
        bar = _tqdm(it, total=n, disable=not (self.opts.progress and self.rank == 0))
        if self.optimizer is not None:
            self.optimizer.zero_grad()
        for i, (inputs, targets) in enumerate(bar):
            inputs = inputs.to(self.device, non_blocking=True)
            targets = targets.to(self.device, non_blocking=True)
            boundary = ((i + 1) % acc_steps == 0) or (i + 1 == n)
            loss, outputs = self._forward_backward(inputs, targets, sync=boundary)
            if boundary:
                self._optimizer_step()
                if self.optimizer is not None:
                    self.optimizer.zero_grad()
            if self.scheduler_type == "CosineAnnealingWarmRestarts":
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    self.scheduler.step(epoch - 1 + i / n)
            running_loss += loss.detach().double()
            if self.metric:
                running_metric += self._evaluate(self._metric_outputs(outputs), targets).double()
            samples += inputs.shape[0]
            if self.opts.log_interval and (i + 1) % self.opts.log_interval == 0:
                bar.set_postfix(loss=running_loss.item() / (i + 1))
            if self._watchdog:
                self._watchdog.beat()
        bar.close()
        loss = running_loss.item() / max(n, 1)
        metric = running_metric.item() / max(n, 1) if self.metric else None
        return loss, metric, samples

    # ------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def evaluate(self, loader=None, model=None):
        """Loss (and metric) over ``loader`` (default: the validation loader).
        Returns ``(loss, metric)`` when a metric is configured, else ``loss``."""
        loader = loader if loader is not None else self.val_loader
        model = model if model is not None else self.model
        n = len(loader)
        if model is self.model and loader is getattr(self, "val_loader", None) and self._engine_eligible(True):
            eng = self._get_val_engine()
            idx = torch.randperm(len(loader.dataset)).to(torch.int32)
            eng.start_epoch(idx)
            eng.ctrl[0:1].fill_(len(self.val_losses) * 1_000_003)
            eng.reset_stats()
            full, last = divmod(idx.numel(), self.batch_size)
            eng.eval_steps(self.batch_size, full)
            if last:
                eng.eval_steps(last, 1)
            loss, acc = eng.read_stats(n)
            return (loss, acc) if self.metric else loss
        was_training = model.training
        model.eval()
        running_loss = torch.zeros((), dtype=torch.float64, device=self.device)
        running_metric = torch.zeros((), dtype=torch.float64, device=self.device)
        it = self._device_batches(loader, train=False) if model is self.model else (
            DevicePrefetcher(loader, self.device) if self.device.type == "cuda" else loader)
        for inputs, targets in _tqdm(it, total=n, disable=not (self.opts.progress and self.rank == 0)):
            inputs = inputs.to(self.device, non_blocking=True)
            targets = targets.to(self.device, non_blocking=True)
            outputs = model(inputs)
            running_loss += self.criterion(outputs, targets).detach().double()
            if self.metric:
                running_metric += self._evaluate(self._metric_outputs(outputs), targets).double()
        if was_training:
            model.train()
        loss = running_loss.item() / max(n, 1)
        if self.metric:
            return loss, running_metric.item() / max(n, 1)
        return loss

    def _validate_one_epoch(self):
        with range_ctx("validate", self.opts.profile_ranges):
            res = self.evaluate(self.val_loader)
        loss, metric = res if self.metric else (res, None)
        if self.opts.global_metrics and mdist.is_dist():
            loss, metric = self._global_mean(loss, metric)
        self.val_losses.append(loss)
        if self.metric:
            self.val_metrics.append(metric)

    def test(self, model, test_loader):
        """Evaluate ``model`` on ``test_loader`` (reference src/trainer.py:277-301; now under
        eval()/no_grad, B13). Returns ``(loss, metric)`` or ``loss``."""
        logger.info("Testing..")
        model = model.to(self.device)
        return self.evaluate(test_loader, model=model)

    # ------------------------------------------------------------------ artifacts
    def save_model(self, model_dir, trainer_state=None):
        """model.pth (+ trainer_state.pt when given). With ``async_checkpoint`` both are written by
        a background thread from host snapshots taken here, model.pth first."""
        logger.info("Saving the model.")
        if self.opts.async_checkpoint:
            if getattr(self, "_ackpt", None) is None:
                self._ackpt = ckpt.AsyncCheckpointer()
            path = os.path.join(model_dir, "model.pth")
            extra = [] if trainer_state is None else [(os.path.join(model_dir, "trainer_state.pt"),
                                                       ckpt.to_host(trainer_state))]
            self._ackpt.save(self.model, path, extra)
            if not getattr(self, "_in_fit", False):
                # a direct call (the reference API) returns with the files on disk and any write
                # error raised; inside fit() they are on disk by the next save / the end of fit()
                self._ackpt.wait()
            return path
        path = ckpt.save_model_file(self.model, model_dir)
        if trainer_state is not None:
            ckpt.save_trainer_state(trainer_state, model_dir)
        return path

    def _checkpoint_wait(self) -> None:
        if getattr(self, "_ackpt", None) is not None:
            self._ackpt.wait()

    def save_history_(self, model_dir):
        logger.info("Saving the training history.")
        return ckpt.save_history_file(self.history, model_dir)

    def _trainer_state(self, epoch: int) -> Dict[str, Any]:
        st = {"epoch": epoch, "global_step": self.global_step,
              "train_losses": self.train_losses, "val_losses": self.val_losses,
              "train_metrics": self.train_metrics, "val_metrics": self.val_metrics,
              "torch_rng": torch.get_rng_state(),
              "py_rng": list(random.getstate()[1]), "py_rng_pos": random.getstate()[2]}
        if self.optimizer is not None:
            st["optimizer"] = self.optimizer.state_dict()
        if self.scheduler is not None:
            st["scheduler"] = self.scheduler.state_dict()
        if self.device.type == "cuda":
            st["cuda_rng"] = torch.cuda.get_rng_state()
        return st

    def _resume(self) -> None:
        path = os.path.join(self.model_dir, "model.pth")
        st = ckpt.load_trainer_state(self.model_dir)
        if not os.path.exists(path) or st is None:
            logger.warning("resume requested but no checkpoint found", model_dir=self.model_dir)
            return
        sd = torch.load(path, map_location="cpu", weights_only=True)
        # checkpoints of wrapped (module.-prefixed) and unwrapped runs both resume either way
        self._core.load_state_dict(ckpt.strip_module_prefix(sd))
        if self.flat is not None:
            self.flat.rebind_params()
        if self._zero is not None:
            self._zero.shard.load_from_full()
        if self.optimizer is not None and "optimizer" in st:
            self.optimizer.load_state_dict(st["optimizer"])
        if self.scheduler is not None and "scheduler" in st:
            self.scheduler.load_state_dict(st["scheduler"])
        self.train_losses, self.val_losses = list(st["train_losses"]), list(st["val_losses"])
        self.train_metrics, self.val_metrics = list(st["train_metrics"]), list(st["val_metrics"])
        self.global_step = int(st["global_step"])
        self.start_epoch = int(st["epoch"]) + 1
        torch.set_rng_state(st["torch_rng"])
        if "cuda_rng" in st and self.device.type == "cuda":
            torch.cuda.set_rng_state(st["cuda_rng"])
        random.setstate((3, tuple(st["py_rng"]), st["py_rng_pos"]))
        logger.info("Resumed training.", epoch=self.start_epoch, global_step=self.global_step)

    def _checkpoint(self, epoch: int) -> None:
        if self.is_parallel and mdist.is_dist():
            # ZeRO: gathering the sharded optimizer state is collective, so every rank builds it
            st = self._trainer_state(epoch) if (self.opts.save_trainer_state and self._zero is not None) else None
            if mdist.rank() == 0:
                if self.opts.save_trainer_state and st is None:
                    st = self._trainer_state(epoch)
                self.save_model(self.model_dir, st if self.opts.save_trainer_state else None)
            # reference has no barrier after the rank-0 save; with async_checkpoint it
            # publishes the host snapshot (the files land in the background, on disk by the next
            # save / the end of fit(), whose wait re-raises a write error)
            mdist.barrier()
        else:
            self.save_model(self.model_dir, self._trainer_state(epoch) if self.opts.save_trainer_state else None)

    def _global_mean(self, loss, metric):
        vals = mdist.all_reduce_scalars([loss, metric if metric is not None else 0.0], "sum")
        w = mdist.world_size()
        return vals[0] / w, (vals[1] / w if metric is not None else None)

    def _determinism_check(self) -> None:
        if not (self.opts.determinism_check and mdist.is_dist() and self.flat is not None):
            return
        # bitwise digest of the raw parameter words (two 31-bit position-weighted sums mod primes,
        # utils/flat.py): a flipped bit or two swapped values on one rank changes it, where a float
        # sum can miss both. Exact integers (< 2^31) compare exactly as the collective's float64.
        from ml_trainer_amd.utils.flat import bitwise_digest
        d = [float(v) for v in bitwise_digest(self.flat.data)]
        lo = mdist.all_reduce_scalars(d, "min")
        hi = mdist.all_reduce_scalars(d, "max")
        if lo != hi:
            raise RuntimeError(f"parameters diverged across ranks (digest min {lo} != max {hi})")

    def fit(self):
        logger.info("Start training..")
        if self._watchdog:
            self._watchdog.start()
        self._in_fit = True
        ok = False  # (not sys.exc_info(): a fit() called inside a caller's except block sees theirs)
        try:
            for epoch in range(self.start_epoch, self.epochs + 1):
                logger.info(f"{'-' * 30} EPOCH {epoch} / {self.epochs} {'-' * 30}")
                self._train_one_epoch(epoch)
                self.clear()
                with self._no_step_phase():
                    self._validate_one_epoch()
                self.clear()
                if self.scheduler_type == "ReduceLROnPlateau":
                    self.scheduler.step(self.val_losses[-1])  # B8 fix: the reference never steps it
                with self._no_step_phase():
                    self._determinism_check()
                    self._checkpoint(epoch)
                if self.metric:
                    logger.info(f"train loss: {self.train_losses[-1]} - "
                                f"train {self.metric}: {self.train_metrics[-1]}")
                    logger.info(f"valid loss: {self.val_losses[-1]} - "
                                f"valid {self.metric}: {self.val_metrics[-1]}\n\n")
                else:
                    logger.info(f"train loss: {self.train_losses[-1]}")
                    logger.info(f"valid loss: {self.val_losses[-1]}\n\n")
                self._write_metrics(epoch)
            ok = True
        finally:
            self._in_fit = False
            if self._watchdog:
                self._watchdog.stop()
            if ok:
                self._checkpoint_wait()  # the last async model.pth is on disk when fit() returns
            else:
                # training already failed: wait for the pending write, but let the ORIGINAL
                # exception propagate (a write error is logged, not raised over it)
                try:
                    self._checkpoint_wait()
                except Exception as e:  # noqa: BLE001
                    logger.warning("checkpoint write failed while handling an earlier error", error=repr(e))
        self.history = {
            "epochs": [*range(1, self.epochs + 1)],
            "train_loss": self.train_losses,
            "val_loss": self.val_losses,
            "train_metric": self.train_metrics,
            "val_metric": self.val_metrics,
            "metric_type": self.metric,
        }
        if self.save_history and (not mdist.is_dist() or mdist.rank() == 0):
            self.save_history_(self.model_dir)
        logger.info("Training Complete.")

    def _write_metrics(self, epoch: int) -> None:
        if not self.opts.metrics_jsonl or self.rank != 0:
            return
        rec = {"epoch": epoch, "train_loss": self.train_losses[-1], "val_loss": self.val_losses[-1],
               "train_metric": self.train_metrics[-1] if self.metric else None,
               "val_metric": self.val_metrics[-1] if self.metric else None,
               **{k: v for k, v in self.throughput[-1].items() if k != "epoch"}}
        os.makedirs(os.path.dirname(os.path.abspath(self.opts.metrics_jsonl)), exist_ok=True)
        with open(self.opts.metrics_jsonl, "a") as f:
            f.write(json.dumps(rec) + "\n")

    def clear(self):
        gc.collect()
        if torch.cuda.is_available():
            torch.cuda.empty_cache()

    def validate_kwargs(self, kwargs, allowed_kwargs, error_message="Keyword argument not understood:"):
        """Checks that all keyword arguments are in the set of allowed keys."""
        for kwarg in kwargs:
            if kwarg not in allowed_kwargs:
                raise TypeError(error_message, kwarg)

    def _no_step_phase(self):
        """Validation / checkpoint: pause the watchdog's no-progress timer (probes stay on)."""
        return self._watchdog.paused() if self._watchdog is not None else _nullctx()


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
