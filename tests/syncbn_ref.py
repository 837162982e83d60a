"""Reference pieces of the cross-rank batch norm tests (no tests here).

RefPhases: the four phases of mmt_amd.train.sync_batchnorm_relu in plain fp64 torch on NHWC tensors [..][pitch]
with C valid channels (CPU or GPU), folding the ranks in rank order with the kernel's merge formula.
full_batch_reference: nn.BatchNorm2d(...).double() in train mode -> ReLU under autograd on the concatenated batch.
"""
import torch


class RefPhases:
    @staticmethod
    def stats(x, C):
        v = x.reshape(-1, x.shape[-1])[:, :C].double()
        mean = v.mean(0)
        var = ((v - mean) ** 2).mean(0)
        return torch.stack([mean, var, torch.full_like(mean, float(v.shape[0]))])

    @staticmethod
    def fold(gathered, W):
        """[W * 3][C] -> (mean, biased variance, count) over the ranks, rank 0's triple first and unchanged."""
        g = gathered.view(W, 3, -1)
        mean, var, n = g[0, 0].clone(), g[0, 1].clone(), g[0, 2].clone()
        for r in range(1, W):
            mr, vr, nr = g[r, 0], g[r, 1], g[r, 2]
            d, N = mr - mean, n + nr
            var = (n * var + nr * vr) / N + d * d * n * nr / (N * N)
            mean = mean + d * nr / N
            n = N
        return mean, var, n

    @staticmethod
    def apply(x, C, gathered, W, weight, bias, running_mean, running_var, momentum, eps):
        mean, var, n = RefPhases.fold(gathered, W)
        if running_mean is not None:
            with torch.no_grad():
                running_mean.mul_(1 - momentum).add_(momentum * mean.to(running_mean.dtype))
                vu = torch.where(n > 1, var * n / (n - 1), var)
                running_var.mul_(1 - momentum).add_(momentum * vu.to(running_var.dtype))
        inv = 1.0 / torch.sqrt(var + eps)
        sc = (weight.double() if weight is not None else torch.ones_like(inv)) * inv
        sh = (bias.double() if bias is not None else torch.zeros_like(inv)) - mean * sc
        save = torch.stack([mean, inv, sc, sh])
        y = torch.zeros_like(x)
        y[..., :C] = torch.relu(x[..., :C].double() * sc + sh).to(x.dtype)
        return y, save, n[:1].clone()

    @staticmethod
    def _g_xhat(x, dy, C, save):
        v = x[..., :C].double()
        g = torch.where(v * save[2] + save[3] > 0, dy[..., :C].double(), torch.zeros((), dtype=torch.float64, device=x.device))
        return g, (v - save[0]) * save[1]

    @staticmethod
    def bwd_sums(x, dy, C, save):
        g, xh = RefPhases._g_xhat(x, dy, C, save)
        sums = torch.stack([(g * xh).reshape(-1, C).sum(0), g.reshape(-1, C).sum(0)])
        return sums.clone(), sums

    @staticmethod
    def bwd_dx(x, dy, C, weight, save, sums, n_total):
        g, xh = RefPhases._g_xhat(x, dy, C, save)
        k = (weight.double() if weight is not None else 1.0) * save[1]
        dx = torch.zeros_like(x)
        dx[..., :C] = (k * (g - sums[1] / n_total - xh * (sums[0] / n_total))).to(x.dtype)
        return dx


def full_batch_reference(x, dy, weight, bias, running_mean, running_var, momentum, eps):
    """x / dy [N][H][W][C] (the ranks' batches concatenated; any float dtype) -> fp64 (y, dx, dgamma, dbeta,
    running_mean, running_var, batch mean, batch invstd) of nn.BatchNorm2d in train mode -> ReLU."""
    C = x.shape[-1]
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=momentum).double()
    with torch.no_grad():
        bn.weight.copy_(weight.double())
        bn.bias.copy_(bias.double())
        bn.running_mean.copy_(running_mean.double())
        bn.running_var.copy_(running_var.double())
    bn.train()
    xr = x.detach().double().cpu().requires_grad_(True)
    y = torch.relu(bn(xr.permute(0, 3, 1, 2))).permute(0, 2, 3, 1)
    y.backward(dy.detach().double().cpu())
    v = xr.detach().reshape(-1, C)
    mean = v.mean(0)
    inv = 1.0 / torch.sqrt(((v - mean) ** 2).mean(0) + eps)
    return {"y": y.detach(), "dx": xr.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
            "running_mean": bn.running_mean.clone(), "running_var": bn.running_var.clone(),
            "mean": mean, "invstd": inv, "tracked": int(bn.num_batches_tracked)}
