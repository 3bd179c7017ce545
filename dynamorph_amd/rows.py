"""Rows on their way to the device, for the analysis layer (pca, knn, kmeans, umap_layout): which device, what shape, host
data as a tensor, and device_chunks -- the one loop that hands a consumer fp32 device chunks of a matrix that lies on the
device already or is streamed from the host through pinned staging and two device buffers."""
import numpy as np
import torch


def device_of(X, device=None):
    """The device of a CUDA tensor X; otherwise `device`, or the current CUDA device where that is None."""
    if torch.is_tensor(X) and X.is_cuda:
        return X.device
    return torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())


def shape_of(X):
    """The shape of a tensor, an array or nested lists, from the shape alone: nothing moves."""
    return tuple(X.shape) if hasattr(X, "shape") else np.shape(X)


def host_rows(X, what="PCA"):
    """Host data as a 2-D torch tensor (a view when it can be); a tensor, on any device, is returned as it is."""
    if isinstance(X, np.ndarray):
        X = torch.from_numpy(X if X.dtype in (np.float32, np.float64) else X.astype(np.float32))
    elif not torch.is_tensor(X):
        X = torch.as_tensor(np.asarray(X, dtype=np.float32))
    if X.dim() != 2:
        raise ValueError(f"{what} expects a 2-D (samples, features) array, got shape {tuple(X.shape)}")
    return X


def chunk_size(chunk_rows, N, F=1, max_chunk_bytes=None):
    """Rows per chunk: at most chunk_rows, N and max_chunk_bytes of fp32 rows of F features, at least one."""
    cr = min(int(chunk_rows), N)
    if max_chunk_bytes is not None:
        cr = min(cr, max_chunk_bytes // (4 * F))
    return max(1, cr)


def device_chunks(X, chunk_rows, device=None, max_chunk_bytes=None):
    """Yields (lo, chunk) over the rows of X (N, F) in order: chunk is rows lo .. lo + m of X as an fp32 matrix on the
    device with unit column stride, m <= chunk_size(chunk_rows, N, F, max_chunk_bytes).  The caller holds the device
    (torch.cuda.device) and no_grad, and enqueues what reads the chunk on the current stream before it asks for the next.

    X on the device is sliced in place (converted or made contiguous once).  Host X is streamed: a chunk is staged in pinned
    memory (skipped for pinned contiguous fp32) and copied on a stream of its own into one of two device buffers, so the
    next chunk's copy overlaps the current chunk's kernels; the current stream waits for the copy before the chunk is
    yielded, and the copy that reuses a buffer waits for the kernels that read it."""
    if torch.is_tensor(X) and X.is_cuda:
        x = X if X.dtype == torch.float32 else X.float()
        if x.shape[1] > 1 and x.stride(1) != 1:
            x = x.contiguous()
        cr = chunk_size(chunk_rows, x.shape[0], x.shape[1], max_chunk_bytes)
        for lo in range(0, x.shape[0], cr):
            yield lo, x[lo:lo + cr]
        return
    X = host_rows(X)
    N, F = X.shape
    dev = device_of(X, device)
    cr = chunk_size(chunk_rows, N, F, max_chunk_bytes)
    compute = torch.cuda.current_stream(dev)
    s_in = torch.cuda.Stream(dev)
    s_in.wait_stream(compute)       # the fresh buffers may be blocks whose last owner still has work queued on `compute`
    direct = X.dtype == torch.float32 and X.is_contiguous() and X.is_pinned()
    stage = None if direct else [torch.empty((cr, F), dtype=torch.float32, pin_memory=True) for _ in range(2)]
    x_dev = [torch.empty((cr, F), dtype=torch.float32, device=dev) for _ in range(2)]
    ev_in = [torch.cuda.Event() for _ in range(2)]       # chunk has reached x_dev[b] (staging b is free again)
    ev_done = [torch.cuda.Event() for _ in range(2)]     # kernels reading x_dev[b] are done
    for it, lo in enumerate(range(0, N, cr)):
        b = it & 1
        m = min(cr, N - lo)
        src = X[lo:lo + m]
        if not direct:
            ev_in[b].synchronize()
            stage[b][:m].copy_(src)
            src = stage[b][:m]
        with torch.cuda.stream(s_in):
            s_in.wait_event(ev_done[b])
            x_dev[b][:m].copy_(src, non_blocking=True)
            ev_in[b].record(s_in)
        compute.wait_event(ev_in[b])
        yield lo, x_dev[b][:m]
        ev_done[b].record(compute)
