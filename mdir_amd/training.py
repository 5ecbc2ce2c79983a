"""The inner step of the reference's training loop (cirtorch/examples/train.py:350-364) on this package's network and criteria.

Only the step: forward one tuple image by image, evaluate the criterion, back-propagate.  Gradients accumulate in the parameters'
``.grad`` over the tuples of a batch exactly as upstream; the optimiser, the epoch loop, the tuple dataset and its mining
(``mdir_amd.mining``) are the caller's.
"""
import torch


def set_batchnorm_eval(module):
    """For ``model.apply`` after ``model.train()`` (train.py:337): every BatchNorm keeps its running statistics, because a tuple is
    forwarded one image at a time; its scale and shift still learn."""
    if "BatchNorm" in type(module).__name__:
        module.eval()


def tuple_step(net, criterion, images, target):
    """One tuple: ``images`` (S tensors [1,3,H,W] or [3,H,W], any sizes) through ``net`` into the columns of a [D,S] matrix,
    ``criterion(matrix, target)``, ``backward()``.  Returns the loss as a float (one read-back).  The images are moved to the
    device of the network's parameters; ``target`` is the tuple's labels ``(-1, 1, 0, ..)``."""
    device = next(net.parameters()).device
    columns = []
    for image in images:
        x = image.to(device)
        out = net(x if x.dim() == 4 else x.unsqueeze(0))                 # [D, 1]
        columns.append(out.reshape(-1))
    output = torch.stack(columns, dim=1)                                  # [D, S]: the graph of every image hangs on its column
    loss = criterion(output, target)
    loss.backward()
    return float(loss.detach())
