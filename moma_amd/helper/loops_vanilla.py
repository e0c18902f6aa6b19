"""The teacher trainer's loops (reference: helper/loops_moma.py:13-65 `train_vanilla` and the `validate_vanilla` that ends at :444, the two
functions its train_teacher.py:29 wants from a module that does not exist).

Order of operations per batch is the reference's: forward, criterion, metrics, zero_grad, backward, optimizer step, the printed line.
What differs, all performance-only:
  * the criterion is helper.ce_head.CrossEntropyHead with its device meter: the loss, the top-1 count and (in validation) the confusion
    matrix come from the head's two launches, and the two per-step `.item()` reads (reference :41, :45) become one `read()` per
    `print_freq` steps and one at the end.  With `--no_fused` the criterion is nn.CrossEntropyLoss and the metrics are
    helper.util.accuracy, the reference's sequence of operations, their values kept on the device until they are printed;
  * `--amp` autocast, `--channels_last`, the GradScaler of `--amp fp16` and the gradient exchange of learning/ddp.py's flat wrap follow
    helper.loops_moma.train_distill_moma;
  * validation accumulates on the device (the reference gathers every logit on the host) and does not read the host inside its loop;
    under DDP the ranks' sums and matrices are added as in the reference (:427-442)."""
from __future__ import print_function

import sys
import time

import torch

from .ce_head import CrossEntropyHead
from .util import AverageMeter, accuracy
from ..learning.ddp import FlatDataParallel


def _device(opt):
    dev = getattr(opt, "device", None)
    if dev is None:
        dev = torch.device("cuda", opt.gpu if (opt.gpu is not None and opt.multiprocessing_distributed) else 0) \
            if torch.cuda.is_available() else torch.device("cpu")
    return dev


def _autocast(opt):
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(getattr(opt, "amp", None))
    return torch.autocast("cuda", dtype=dtype, enabled=dtype is not None)


def _metered(criterion):
    return isinstance(criterion, CrossEntropyHead) and criterion.meter


def train_vanilla(epoch, train_loader, model, criterion, optimizer, opt):
    """vanilla training; returns (top-1 %, mean loss) like the reference."""
    model.train()
    batch_time, losses, top1 = AverageMeter(), AverageMeter(), AverageMeter()
    n_batch = len(train_loader)
    dev = _device(opt)
    scaler = getattr(opt, "_grad_scaler", None)
    metered = _metered(criterion)
    if metered:
        criterion.reset()
    flat_dp = isinstance(model, FlatDataParallel)
    flat_params = model.grad_params() if flat_dp else None
    trace = getattr(opt, "trace", None)

    end = time.time()
    for idx, (images, labels) in enumerate(train_loader):
        images = images.to(dev, non_blocking=True)
        labels = labels.to(dev, non_blocking=True)
        if getattr(opt, "channels_last", False):
            images = images.contiguous(memory_format=torch.channels_last)

        # ===================forward=====================
        with _autocast(opt):
            output = model(images)
        loss = criterion(output if metered else output.float(), labels)
        if not metered:
            losses.update(loss.detach(), images.size(0))
            # ===================Metrics=====================
            top1.update(accuracy(output, labels, topk=(1,))[0].squeeze(0), images.size(0))
        if trace is not None:           # optional per-step record (tests / benchmarking), device tensors
            trace.append(loss.detach())

        # ===================backward=====================
        optimizer.zero_grad()
        if scaler is not None:
            scaler.scale(loss).backward()
        else:
            loss.backward()
        if flat_dp:
            model.allreduce_grads(flat_params)
        if scaler is not None:
            scaler.step(optimizer)
            scaler.update()
        else:
            optimizer.step()
        batch_time.update(time.time() - end)
        end = time.time()

        # print info
        if idx % opt.print_freq == 0:
            acc, avg = criterion.read()[:2] if metered else (float(top1.avg), float(losses.avg))
            print('Epoch: [{0}][{1}/{2}]\t'
                  'GPU {3}\t'
                  'Time: {batch_time.avg:.3f}\t'
                  'Loss {loss:.4f}\t'
                  'Acc@1 {top1:.3f}'.format(epoch, idx, n_batch, opt.gpu, batch_time=batch_time, loss=avg, top1=acc))
            sys.stdout.flush()
    if metered:
        return criterion.read()[:2]
    return float(top1.avg), float(losses.avg)


def validate_vanilla(val_loader, model, criterion, opt, prefix='Test'):
    """validation; returns (top-1 %, mean loss, {'acc', 'conf_mat'}).  No host read inside the loop."""
    model.eval()
    n_cls = int(opt.n_cls)
    dev = _device(opt)
    metered = _metered(criterion)
    if metered:
        criterion.reset()
        sums, conf = criterion.stats, criterion.conf
    else:
        conf = torch.zeros(n_cls * n_cls, dtype=torch.int64, device=dev)
        sums = torch.zeros(4, dtype=torch.float64, device=dev)          # loss sum, hits, count, -
    t0 = time.time()
    with torch.no_grad():
        for idx, (images, labels) in enumerate(val_loader):
            images = images.to(dev, non_blocking=True)
            labels = labels.to(dev, non_blocking=True)
            if getattr(opt, "channels_last", False):
                images = images.contiguous(memory_format=torch.channels_last)
            with _autocast(opt):
                output = model(images)
            if metered:
                criterion(output, labels)
                continue
            output = output.float()
            n = images.size(0)
            pred = output.argmax(dim=1)
            sums[0] += criterion(output, labels).detach().double() * n
            sums[1] += (pred == labels).sum()
            sums[2] += n
            conf += torch.bincount(labels * n_cls + pred, minlength=n_cls * n_cls)
    if getattr(opt, "multiprocessing_distributed", False) and torch.distributed.is_initialized():
        # (batch sizes may differ between the ranks: sums and counts are added, reference :427-435)
        torch.distributed.all_reduce(sums)
        torch.distributed.all_reduce(conf)
    s = sums.tolist()
    acc, loss = 100.0 * s[1] / max(s[2], 1.0), s[0] / max(s[2], 1.0)
    print('{3}: [{0}/{1}]\t'
          'GPU: {2}\t'
          'Time: {4:.3f}\t'
          'Loss {5:.4f}\t'
          'Acc@1 {6:.3f}'.format(len(val_loader), len(val_loader), opt.gpu, prefix, (time.time() - t0) / max(len(val_loader), 1), loss, acc))
    return acc, loss, {"acc": acc, "conf_mat": conf.view(n_cls, n_cls).cpu().numpy()}
