"""Cross-Layer Distillation with Semantic Calibration (Chen et al., AAAI 2021) -- the criterion of `--distill semckd` (reference
distiller_zoo/SemCKD.py and models/util.py SelfA, Proj, MLPEmbed; built in train_student_moma.py:358-364, loop branch
helper/loops_moma.py:101-102, 177-179).

Every student map of feat_s[1:-1] is compared with every teacher map of feat_t[1:-1]: S x T pairs.  SelfA holds, per student map i, a
query head `query_i` and, per teacher map j, a key head `key_j` (MLPEmbed on the B x B batch Gram matrix of the map, so the module is
built for ONE batch size, `feat_dim`), and per pair a projection `regressor{i}{j}` (Proj: conv1x1 -> BN -> ReLU -> conv3x3 -> BN ->
ReLU -> conv1x1, all bias-free) that takes the student's map to the teacher's channels on the smaller of the two grids.  The softmax
of query . key / soft over j is the attention [B, S, T] that weights the per-sample mean squared errors in SemCKDLoss.
Attribute names, state-dict keys, construction order (so the RNG draws), forward signatures and returns are the reference's.  MLPEmbed
also keeps its `regressor` Sequential, which no forward uses: it draws from the RNG and owns state-dict keys, and its parameters never
get a gradient (the optimizer and both gradient exchanges skip parameters without one).

`SelfA.loss(feat_s, feat_t)` is what the training loop calls: SemCKDLoss(*forward(feat_s, feat_t)) as one value.  On GPU maps in
float32 / bfloat16 the Gram matrices run on csrc/sp.hip (ops.batch_gram), the head (MLPEmbed, bmm / soft, softmax) in float32 with
autocast disabled (Gram entries reach 1e5 and more), each distinct (teacher map, grid) is pooled once without a graph, and all pairs'
weighted errors and their backward run as ONE grouped call each on csrc/semckd.hip (ops.semckd_weighted_mse).  Proj's 1 x 1
convolutions are backbones.efficientnet.SamePadConv2d, so under bf16 autocast they reach csrc/pwstream.hip where
ops.pwconv_fwd_native admits the layer; its BatchNorm, ReLU and 3 x 3 convolution are stock.
CPU tensors, float16 / float64 storage, odd strides and more than 64 pairs take `composite`: the same formula in stock torch ops,
evaluated in float64 and returned in float32.  The formula needs [B, C, H, W] maps: token lists (the ViT backbones) are refused."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..backbones.efficientnet import SamePadConv2d

_KERNEL_DTYPES = (torch.float32, torch.bfloat16)


def _dense(f):
    return f.is_contiguous() or f.is_contiguous(memory_format=torch.channels_last)


def _refuse_tokens(feats):
    for f in feats:
        if f.dim() != 4:
            raise ValueError("SemCKD compares [B, C, H, W] feature maps; got {} (the token lists of a ViT backbone have no grid for "
                             "the projections' convolutions)".format(tuple(f.shape)))


class SemCKDLoss(nn.Module):
    """Cross-Layer Distillation with Semantic Calibration, AAAI2021"""

    def __init__(self):
        super().__init__()
        self.crit = nn.MSELoss(reduction='none')

    def forward(self, s_value, f_target, weight):
        bsz, num_stu, num_tea = weight.shape
        ind_loss = torch.zeros(bsz, num_stu, num_tea, device=weight.device)
        for i in range(num_stu):
            for j in range(num_tea):
                ind_loss[:, i, j] = self.crit(s_value[i][j], f_target[i][j]).reshape(bsz, -1).mean(-1)
        loss = (weight * ind_loss).sum() / (1.0 * bsz * num_stu)
        return loss


class Normalize(nn.Module):
    """normalization layer"""

    def __init__(self, power=2):
        super().__init__()
        self.power = power

    def forward(self, x):
        norm = x.pow(self.power).sum(1, keepdim=True).pow(1. / self.power)
        out = x.div(norm)
        return out


class MLPEmbed(nn.Module):
    """non-linear mapping for attention calculation"""

    def __init__(self, dim_in=1024, dim_out=128):
        super().__init__()
        self.linear1 = nn.Linear(dim_in, 2 * dim_out)
        self.relu = nn.ReLU(inplace=True)
        self.linear2 = nn.Linear(2 * dim_out, dim_out)
        self.l2norm = Normalize(2)
        self.regressor = nn.Sequential(          # (the reference's: never used by forward, but it draws from the RNG and owns keys)
            nn.Linear(dim_in, 2 * dim_out),
            self.l2norm,
            nn.ReLU(inplace=True),
            nn.Linear(2 * dim_out, dim_out),
            self.l2norm,
        )

    def forward(self, x):
        x = x.view(x.shape[0], -1)
        x = self.relu(self.linear1(x))
        x = self.l2norm(self.linear2(x))
        return x


class Proj(nn.Module):
    """feature dimension alignment by 1x1, 3x3, 1x1 convolutions"""

    def __init__(self, num_input_channels=1024, num_target_channels=128):
        super().__init__()
        self.num_mid_channel = 2 * num_target_channels

        def conv1x1(in_channels, out_channels):
            return SamePadConv2d(in_channels, out_channels, 1, bias=False)

        def conv3x3(in_channels, out_channels, stride=1):
            return nn.Conv2d(in_channels, out_channels, kernel_size=3, padding=1, stride=stride, bias=False)

        self.regressor = nn.Sequential(
            conv1x1(num_input_channels, self.num_mid_channel),
            nn.BatchNorm2d(self.num_mid_channel),
            nn.ReLU(inplace=True),
            conv3x3(self.num_mid_channel, self.num_mid_channel),
            nn.BatchNorm2d(self.num_mid_channel),
            nn.ReLU(inplace=True),
            conv1x1(self.num_mid_channel, num_target_channels),
        )

    def forward(self, x):
        x = self.regressor(x)
        return x


class SelfA(nn.Module):
    """Cross-layer Self Attention"""

    def __init__(self, feat_dim, s_n, t_n, soft, factor=4):
        super().__init__()
        self.soft = soft
        self.s_len = len(s_n)
        self.t_len = len(t_n)
        self.feat_dim = feat_dim

        # query and key mapping
        for i in range(self.s_len):
            setattr(self, 'query_' + str(i), MLPEmbed(feat_dim, feat_dim // factor))
        for i in range(self.t_len):
            setattr(self, 'key_' + str(i), MLPEmbed(feat_dim, feat_dim // factor))

        for i in range(self.s_len):
            for j in range(self.t_len):
                setattr(self, 'regressor' + str(i) + str(j), Proj(s_n[i], t_n[j]))

    def _check(self, feat_s, feat_t):
        if len(feat_s) != self.s_len or len(feat_t) != self.t_len:
            raise ValueError("SelfA was built for {} student and {} teacher maps, got {} and {}".format(
                self.s_len, self.t_len, len(feat_s), len(feat_t)))
        _refuse_tokens(list(feat_s) + list(feat_t))
        for f in list(feat_s) + list(feat_t):
            if f.shape[0] != self.feat_dim:
                raise ValueError("SelfA was built for batches of {} (its query and key heads read the {} x {} batch Gram matrix); got a "
                                 "batch of {} (the loop skips a shorter last batch)".format(self.feat_dim, self.feat_dim, self.feat_dim,
                                                                                            f.shape[0]))

    def _attention(self, sim_s, sim_t):
        """the head: query_i / key_j on the Gram matrices, bmm / soft, softmax over the teacher maps -> [B, S, T]"""
        proj_query = torch.stack([getattr(self, 'query_' + str(i))(sim_s[i]) for i in range(self.s_len)], 1)
        proj_key = torch.stack([getattr(self, 'key_' + str(j))(sim_t[j]) for j in range(self.t_len)], 2)
        energy = torch.bmm(proj_query, proj_key) / self.soft
        return F.softmax(energy, dim=-1)

    def forward(self, feat_s, feat_t):
        self._check(feat_s, feat_t)
        bsz = self.feat_dim
        sim_s, sim_t = [], []
        for f in feat_s:
            sim_temp = f.reshape(bsz, -1)
            sim_s.append(torch.matmul(sim_temp, sim_temp.t()))
        for f in feat_t:
            sim_temp = f.reshape(bsz, -1)
            sim_t.append(torch.matmul(sim_temp, sim_temp.t()))
        attention = self._attention(sim_s, sim_t)

        # feature dimension alignment
        proj_value_stu = []
        value_tea = []
        for i in range(self.s_len):
            proj_value_stu.append([])
            value_tea.append([])
            for j in range(self.t_len):
                s_H, t_H = feat_s[i].shape[2], feat_t[j].shape[2]
                if s_H > t_H:
                    source = F.adaptive_avg_pool2d(feat_s[i], (t_H, t_H))
                    target = feat_t[j]
                else:
                    source = feat_s[i]
                    target = F.adaptive_avg_pool2d(feat_t[j], (s_H, s_H))
                proj_value_stu[i].append(getattr(self, 'regressor' + str(i) + str(j))(source))
                value_tea[i].append(target)
        return proj_value_stu, value_tea, attention

    def takes_kernels(self, feat_s, feat_t):
        """whether the Gram matrices and the weighted errors of this call run on csrc/sp.hip and csrc/semckd.hip"""
        maps = list(feat_s) + list(feat_t)
        return (ops.semckd_native(self.s_len * self.t_len) and self.feat_dim <= 1024
                and all(f.is_cuda and f.dtype in _KERNEL_DTYPES and f.dim() == 4 and _dense(f) and f.numel() > 0 for f in maps)
                and not any(t.requires_grad and torch.is_grad_enabled() for t in feat_t)
                and all(p.is_cuda and p.dtype == torch.float32 for p in self.parameters()))

    def loss(self, feat_s, feat_t):
        """SemCKDLoss(*self.forward(feat_s, feat_t)) -> scalar float32"""
        self._check(feat_s, feat_t)
        if not self.takes_kernels(feat_s, feat_t):
            return self.composite(feat_s, feat_t)
        dev_type = feat_s[0].device.type
        sim_s = [ops.batch_gram(f) for f in feat_s]
        with torch.no_grad():
            sim_t = [ops.batch_gram(f) for f in feat_t]
        with torch.autocast(dev_type, enabled=False):
            attention = self._attention(sim_s, sim_t)
        pooled = {}                                   # (teacher map, grid) -> the target, pooled once and reused across i
        s_value, targets = [], []
        for i in range(self.s_len):
            s_value.append([])
            targets.append([])
            for j in range(self.t_len):
                s_H, t_H = feat_s[i].shape[2], feat_t[j].shape[2]
                if s_H > t_H:
                    source, h = F.adaptive_avg_pool2d(feat_s[i], (t_H, t_H)), None     # (the teacher's map as it is)
                else:
                    source, h = feat_s[i], s_H
                y = getattr(self, 'regressor' + str(i) + str(j))(source)
                if y.dtype not in _KERNEL_DTYPES or not _dense(y):
                    return self.composite(feat_s, feat_t)
                fmt = torch.contiguous_format if y.is_contiguous() else torch.channels_last
                key = (j, h, fmt)
                if key not in pooled:
                    with torch.no_grad():
                        t = feat_t[j] if h is None else F.adaptive_avg_pool2d(feat_t[j], (h, h))
                        # a target in the other memory format than the projection's output is copied into that format once
                        pooled[key] = t.detach().contiguous(memory_format=fmt)
                s_value[i].append(y)
                targets[i].append(pooled[key])
        loss, _ = ops.semckd_weighted_mse(s_value, targets, attention)
        return loss

    def composite(self, feat_s, feat_t, dtype=torch.float64):
        """the same value in stock torch ops: the Gram matrices, the head and the weighted errors evaluated in `dtype` (the projections
        run as they are, under the caller's autocast), returned in float32 (float64 maps: in float64)"""
        self._check(feat_s, feat_t)
        dev_type = feat_s[0].device.type
        with torch.autocast(dev_type, enabled=False):
            sims = []
            for f in list(feat_s) + list(feat_t):
                x = f.reshape(self.feat_dim, -1).to(dtype)
                sims.append(x @ x.t())
            heads = [getattr(self, 'query_' + str(i)) for i in range(self.s_len)] + [getattr(self, 'key_' + str(j)) for j in range(self.t_len)]
            emb = []
            for m, g in zip(heads, sims):
                h = F.relu(F.linear(g, m.linear1.weight.to(dtype), m.linear1.bias.to(dtype)))
                emb.append(m.l2norm(F.linear(h, m.linear2.weight.to(dtype), m.linear2.bias.to(dtype))))
            query, key = torch.stack(emb[:self.s_len], 1), torch.stack(emb[self.s_len:], 2)
            weight = F.softmax(torch.bmm(query, key) / self.soft, dim=-1)
        total = 0.0
        for i in range(self.s_len):
            for j in range(self.t_len):
                s_H, t_H = feat_s[i].shape[2], feat_t[j].shape[2]
                if s_H > t_H:
                    source, target = F.adaptive_avg_pool2d(feat_s[i], (t_H, t_H)), feat_t[j]
                else:
                    source, target = feat_s[i], F.adaptive_avg_pool2d(feat_t[j], (s_H, s_H))
                y = getattr(self, 'regressor' + str(i) + str(j))(source)
                with torch.autocast(dev_type, enabled=False):
                    ind = ((y.to(dtype) - target.to(dtype)) ** 2).reshape(self.feat_dim, -1).mean(-1)
                    total = total + (weight[:, i, j] * ind).sum()
        out = total / (1.0 * self.feat_dim * self.s_len)
        return out if feat_s[0].dtype == torch.float64 else out.float()
