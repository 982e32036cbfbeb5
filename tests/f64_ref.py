"""float64 evaluation of one training step's loss and gradients (test infrastructure): the reference's Linear/ReLU chain
and mean-squared error in torch float64, on whatever device the caller picks."""
import numpy as np
import torch


def float64_grads(params, relu_flags, x, fmask, device):
    """(loss, [(dW, db)] as float64 numpy) of mse_mean(x, chain(x * fmask)) - the step EmbeddingTrainer.step takes."""
    xt = torch.tensor(np.asarray(x), dtype=torch.float64, device=device)
    h = xt * torch.tensor(np.asarray(fmask), dtype=torch.float64, device=device)
    Ws = [torch.tensor(w, dtype=torch.float64, device=device, requires_grad=True) for w, _ in params]
    bs = [torch.tensor(b, dtype=torch.float64, device=device, requires_grad=True) for _, b in params]
    for W, b, relu in zip(Ws, bs, relu_flags):
        h = h @ W.T + b
        if relu:
            h = torch.relu(h)
    loss = ((h - xt) ** 2).mean()
    loss.backward()
    return float(loss), [(W.grad.cpu().numpy(), b.grad.cpu().numpy()) for W, b in zip(Ws, bs)]


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
