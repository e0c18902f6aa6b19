"""Reference arithmetic of the BN1 + activation -> squeeze-excite gate pair in stock torch ops, for tests/test_bn_se_fused_cpu.py
(fp64 on the CPU) and tests/test_gpu_bn_se_fused.py (fp64 on the GPU).  Not collected by pytest (no test_ prefix).

composite()          the chain itself: G = act(BN(D)) * sigmoid(s), s a linear map of the plane means of act(BN(D))
decomposed_grads()   its gradients the way bnse.hip forms them: five sums per plane from (D, dG) alone, the gradient of the plane
                     means from ds, then the channel sums from the plane sums -- no gradient of the activation in between"""
import torch


# Scale of the map from the plane means to the gate logits.  The GPU test checks dgamma / dbeta with the ABSOLUTE tolerances of
# test_bn_act_with_plane_mean, which were set for a gradient of the plane means of about 3 (three times a unit normal), handed
# to the op exactly.  Here that gradient is SCALE * M^T ds with rows of M of unit norm and ds = sigmoid'(s) * sum_hw dG * A1, up
# to 0.25 * sqrt(56 * 56) = 14 at the largest plane of the test: 0.25 keeps it at the scale those tolerances were made for
# (with the 3.0 of test_se_gate_and_plane_mean_match_torch it reached 40, and the bf16 rounding of it alone, outside the code under
# test, used up the tolerance -- for the unfused chain as well).
SCALE = 0.25


def smap(pooled, M):
    """stand-in for the two 1 x 1 convolutions of the squeeze-excite block: [N,C,1,1] -> [N,C,1,1], a small linear map"""
    return torch.einsum("oc,nchw->nohw", M.to(pooled.dtype), pooled) * SCALE


def _act(y, act):
    return torch.nn.functional.silu(y) if act == "silu" else y


def _act_grad(y, act):
    if act != "silu":
        return torch.ones_like(y)
    sg = torch.sigmoid(y)
    return sg * (1 + y * (1 - sg))


def statistics(D, rm, rv, training, eps):
    """(mean, invstd) per channel as [1,C,1,1]: of the batch (biased variance) when training, the running ones otherwise"""
    if training:
        mean = D.mean((0, 2, 3), keepdim=True)
        var = (D - mean).square().mean((0, 2, 3), keepdim=True)
    else:
        mean, var = rm.view(1, -1, 1, 1).to(D.dtype), rv.view(1, -1, 1, 1).to(D.dtype)
    return mean, (var + eps).rsqrt()


def composite(D, gamma, beta, rm, rv, M, training, act, eps):
    """-> (G, pooled, s) in D's dtype, differentiable in D, gamma, beta and M"""
    mean, invstd = statistics(D, rm, rv, training, eps)
    y = (D - mean) * invstd * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    A = _act(y, act)
    pooled = A.mean((2, 3), keepdim=True)
    s = smap(pooled, M)
    return A * torch.sigmoid(s), pooled, s


def decomposed_grads(D, gamma, beta, rm, rv, M, dG, training, act, eps):
    """-> (dD, dgamma, dbeta, ds, dM) of sum(G * dG), by the plane-sum decomposition"""
    N, C, H, W = D.shape
    HW = H * W
    mean, invstd = statistics(D.detach(), rm, rv, training, eps)
    g4, b4 = gamma.detach().view(1, -1, 1, 1), beta.detach().view(1, -1, 1, 1)
    xh = (D.detach() - mean) * invstd
    y = xh * g4 + b4
    A, dA = _act(y, act), _act_grad(y, act)
    pooled = A.mean((2, 3), keepdim=True)
    s = smap(pooled, M.detach())
    sg = torch.sigmoid(s)
    # pass 1 over (D, dG): per plane
    ds = sg * (1 - sg) * (dG * A).sum((2, 3), keepdim=True)
    P1 = (dG * dA).sum((2, 3), keepdim=True)
    P2 = dA.sum((2, 3), keepdim=True)
    P3 = (dG * dA * xh).sum((2, 3), keepdim=True)
    P4 = (dA * xh).sum((2, 3), keepdim=True)
    # the squeeze-excite layers' own backward: ds -> dM and the gradient of the plane means
    dM = SCALE * torch.einsum("nohw,nchw->oc", ds, pooled)
    dpl = SCALE * torch.einsum("oc,nohw->nchw", M.detach(), ds)
    # per channel, from the plane sums
    s1 = (sg * P1 + dpl / HW * P2).sum(0, keepdim=True)
    s2 = (sg * P3 + dpl / HW * P4).sum(0, keepdim=True)
    # pass 2 over (D, dG)
    dy = (dG * sg + dpl / HW) * dA
    a = g4 * invstd
    if training:
        dD = a * (dy - s1 / (N * HW) - xh * s2 / (N * HW))
    else:
        dD = a * dy
    return dD, s2.flatten(), s1.flatten(), ds, dM
