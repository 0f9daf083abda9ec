"""The chain files of a run in the reference's HDF5 layouts and their readers (linna_amd.sampler re-exports them)."""
import os

import numpy as np
import torch

from . import h5lite
from .chainstats import DeviceChain, integrated_time


class _OnDisk(object):
    """Placeholder for a chain block that lives in the HDF5 file only (ChainStore drops big blocks once written)."""
    __slots__ = ("n",)

    def __init__(self, n):
        self.n = int(n)

    def __len__(self):
        return self.n


class ChainStore(object):
    """Chain backend in the reference's file formats: ``chemcee_256.h5`` as emcee's ``HDFBackend`` /
    ``Transformbackend`` lay it out (group ``mcmc``: ``chain``, ``chain_transformed``, ``log_prob``,
    ``accepted`` + attributes ``nwalkers``, ``ndim``, ``iteration``, ``has_blobs``; sampler.py:322-368)
    and ``zeus_256.h5`` as ``ZeusTransformCallback`` does (root datasets ``samples``,
    ``chain_transformed``, ``logprob``; sampler.py:556-577), through ``h5lite`` (no h5py in this
    image), plus the ``<name>.txt`` layout the reference's reader accepts as a fallback
    (main.py:166-167, 293-295: rows of ``theta..., log_prob``; ``write_txt=True``).  Files written by the reference load
    the same way, so a run directory started there resumes here."""

    GZIP_LIMIT = 64 << 20           # zeus layout: gzip chunks like the reference below this many bytes per dataset
    MAX_QUEUED = 8                  # device blocks waiting for the writer: a disk slower than the sampler stalls the sampler
                                    # (put blocks) instead of piling chain blocks up in HBM (108 MB each at 4096 walkers)

    def __init__(self, filename, transform=None, write_txt=False):
        self.base = filename[:-3] if filename.endswith(".h5") else filename
        self.layout = "zeus" if os.path.basename(self.base).startswith("zeus") else "emcee"
        self.transform = transform
        self.write_txt = write_txt          # also keep <name>.txt (theta..., log_prob rows) next to the HDF5 file
        self.chain, self.chain_transformed, self.log_prob = [], [], []
        self.accepted = None
        self._flushed = 0
        self._writer, self._queue, self._error = None, None, None
        self._events, self._copy_stream = {}, None
        self._appender, self._appended = None, 0
        self.busy = {"fetch": 0.0, "append": 0.0}      # seconds the two background threads spent working (driver profiles)

    # Incremental flushes run on two background threads in a pipeline: the first brings a block from the device to the
    # host (copy stream of its own, after the event recorded when the block was appended), the second appends it to the
    # HDF5 file (whose bulk writes fan out over a few more threads, h5lite.Appender).  Zipping / writing 7 MB per
    # convergence check (128 walkers) on the sampling thread took as long as the 100 iterations between two checks; at
    # 4096 walkers a block is 2 x 54 MB and one thread doing copy + write in turn sustained a third of the sampling
    # rate.  numpy's file I/O, os.pwrite and the device copies release the GIL; the sampling thread spends its time
    # inside ctypes calls, which release it too.
    def _enqueue(self, path, arrays):
        import queue, threading, time
        if self._writer is None:
            self._queue, self._wqueue = queue.Queue(maxsize=self.MAX_QUEUED), queue.Queue(maxsize=8)

            def fetch():
                while True:
                    item = self._queue.get()
                    try:
                        if item is not None and self._error is None:
                            t0 = time.perf_counter()
                            self._to_host(item[1])                    # device blocks come to the host HERE, off the sampling thread
                            if torch.is_tensor(item[2]):
                                item = (item[0], item[1], self._acc_host(item[2]))
                            self.busy["fetch"] += time.perf_counter() - t0
                    except Exception as e:          # surfaced by the next drain()
                        self._error = e
                    self._wqueue.put(item)
                    if item is None:
                        return

            def work():
                while True:
                    item = self._wqueue.get()
                    try:
                        if item is None:
                            return
                        if self._error is None:
                            t0 = time.perf_counter()
                            self._append_block(item[1], item[2])
                            self.busy["append"] += time.perf_counter() - t0
                    except Exception as e:
                        self._error = e
                    finally:
                        self._queue.task_done()
            self._fetcher = threading.Thread(target=fetch, name="linna-chain-fetch", daemon=True)
            self._writer = threading.Thread(target=work, name="linna-chain-writer", daemon=True)
            self._fetcher.start()
            self._writer.start()
        self._queue.put((path, arrays[0], arrays[1]))

    def _acc_host(self, a):
        if torch.is_tensor(a):
            if a.is_cuda and self._copy_stream is not None:
                with torch.cuda.stream(self._copy_stream):
                    return a.to("cpu", torch.float64).numpy()
            return a.to("cpu", torch.float64).numpy()
        return np.asarray(a, np.float64)

    def _to_host(self, k):
        """Block k as numpy arrays (in place).  Blocks appended as device tensors are copied on a stream of their own,
        after the event recorded when they were appended: the copy neither waits for nor delays the sampling stream.
        The host side is PINNED memory from torch's caching host allocator (54 MB in 1 ms against 6-11 ms into pageable
        memory; the buffers are recycled once a written block has been dropped, see _append_block)."""
        if not torch.is_tensor(self.chain[k]):
            return
        ev = self._events.pop(k, None)
        dev = self.chain[k].device
        if dev.type == "cuda":
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(self._copy_stream):
                if ev is not None:
                    self._copy_stream.wait_event(ev)
                host = []
                for t in (self.chain[k], self.chain_transformed[k], self.log_prob[k]):
                    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                    h.copy_(t, non_blocking=True)
                    host.append(h)
                self._copy_stream.synchronize()
            host = [h.numpy() for h in host]
        else:
            host = [t.numpy() for t in (self.chain[k], self.chain_transformed[k], self.log_prob[k])]
        self.chain[k], self.chain_transformed[k], self.log_prob[k] = host           # (frees the device copies)

    def drain(self):
        """Wait until every part queued so far is on disk."""
        if self._queue is not None:
            self._queue.join()
        if self._error is not None:
            e, self._error = self._error, None
            raise e

    @property
    def h5(self):
        return self.base + ".h5"

    @property
    def npz(self):                                          # consolidated file of earlier versions of this package
        return self.base + ".npz"

    def exists(self):
        return os.path.isfile(self.h5) or os.path.isfile(self.npz) or bool(self._parts(self.base))

    def remove(self):
        self.drain()
        for f in [self.h5, self.npz, self.base + ".txt"] + self._parts(self.base):
            if os.path.isfile(f):
                os.remove(f)

    def append(self, z_block, theta_block, logp_block, accepted):
        # float32 blocks stay float32 (what the device produced; emcee / h5py read either width): half the
        # bytes of every part file and of the final HDF5 file -- at 4096 walkers the chain is 2 x 54 MB per 100 steps
        # Device tensors are kept as they are (no copy on the sampling thread: at 4096 walkers a block is 2 x 54 MB);
        # they come to the host in the writer thread, or at the latest when the arrays are asked for.
        if torch.is_tensor(z_block) and z_block.is_cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(z_block.device))
            self._events[len(self.chain)] = ev
            self.chain.append(z_block); self.chain_transformed.append(theta_block); self.log_prob.append(logp_block)
            self.accepted = accepted.detach().clone() if torch.is_tensor(accepted) else np.asarray(accepted, np.float64)
            return
        keep = lambda a: np.asarray(a) if np.asarray(a).dtype == np.float32 else np.asarray(a, np.float64)
        self.chain.append(keep(z_block))
        self.chain_transformed.append(keep(theta_block))
        self.log_prob.append(keep(logp_block))
        self.accepted = np.asarray(accepted, np.float64)

    # -- the chain file grows in place (h5lite.Appender): one chunk of every dataset per flushed block ------------
    def _names(self):
        return (("samples", "chain_transformed", "logprob") if self.layout == "zeus"
                else ("mcmc/chain", "mcmc/chain_transformed", "mcmc/log_prob"))

    DROP_BYTES = 16 << 20           # blocks of at least this size are dropped from host memory once they are in the file
    CHUNK_ROWS = 100                # steps per HDF5 chunk: the flush cadence (emcee's backend grows its file likewise),
                                    # whatever the length of the first block -- a resumed chain arrives as ONE long block

    def _spec(self, k):
        nw, nd = self.chain[k].shape[1], self.chain[k].shape[2]
        dt = lambda blocks: np.result_type(*[np.asarray(b).dtype for b in blocks if not torch.is_tensor(b)] or [np.float32])
        tails = dict(zip(self._names(), (((nw, nd), dt(self.chain[:k + 1])), ((nw, nd), dt(self.chain_transformed[:k + 1])),
                                         ((nw,), dt(self.log_prob[:k + 1])))))
        for name, (tail, d) in tails.items():
            if self.CHUNK_ROWS * int(np.prod(tail)) * np.dtype(d).itemsize >= 2 ** 32:
                raise h5lite.H5Error("%s: a chunk of %d steps would reach 4 GiB (HDF5 chunk sizes are 32-bit)" % (name, self.CHUNK_ROWS))
        return nw, nd, tails

    def _adopt_existing(self, k):
        """A resumed run: blocks 0..j of this store are the rows the chain file already holds (sampler drivers load the
        file and append it as one block).  When the file is one of ours (extensible datasets) it simply keeps growing:
        nothing is rewritten, nothing can be lost.  Returns True when adopted."""
        if not os.path.isfile(self.h5):
            return False
        try:
            ap = h5lite.Appender.open(self.h5)
        except Exception:
            return False
        names = self._names()
        try:
            if not all(n in ap.ds for n in names) or any(ap.ds[n]["chunk_rows"] != self.CHUNK_ROWS for n in names):
                raise ValueError
            have = ap.nrows(names[0])
            rows, j = 0, 0
            while j <= k and rows < have:
                rows += len(self.chain[j]); j += 1
            if rows != have or have == 0:
                raise ValueError
            self._to_host(j - 1)
            with h5lite.File(self.h5) as f:                      # the block really is what the file ends with
                last = f[names[0]][have - 1:have]
            if not np.array_equal(np.asarray(last)[0], np.asarray(self.chain[j - 1])[-1]):
                raise ValueError
        except Exception:
            ap.close()
            return False
        self._appender, self._appended = ap, j
        return True

    def _start_appender(self, k):
        """The extensible chain file.  A file of ours that already holds the leading blocks is continued in place;
        otherwise a NEW file is built under ``<name>.h5.tmp`` -- the blocks before k (a resumed run: the old rows)
        included -- and takes the old file's place only when it is complete, so a kill at any moment leaves a readable
        chain behind."""
        self._to_host(k)
        if self._adopt_existing(k):
            return
        nw, nd, spec = self._spec(k)
        names = self._names()
        tmp = self.h5 + ".tmp"
        if self.layout == "zeus":
            ap = h5lite.Appender.create(tmp, spec, chunk_rows=self.CHUNK_ROWS)
        else:
            ap = h5lite.Appender.create(tmp, {n.split("/")[1]: v for n, v in spec.items()}, group="mcmc",
                                        group_attrs=dict(version="3.0.2", nwalkers=np.int64(nw), ndim=np.int64(nd), has_blobs=False,
                                                         iteration=np.int64(0)),
                                        fixed={"accepted": np.zeros(nw)}, chunk_rows=self.CHUNK_ROWS)
        for j in range(k):                                          # what came before block k goes in before the swap
            self._to_host(j)
            ap.append({names[0]: self.chain[j], names[1]: self.chain_transformed[j], names[2]: self.log_prob[j]})
        if self.layout != "zeus" and k > 0:
            ap.set_attr("mcmc", "iteration", ap.nrows(names[0]))
        ap.close()
        os.replace(tmp, self.h5)
        self._appender = h5lite.Appender.open(self.h5)
        self._appended = k

    def _append_block(self, k, accepted):
        if self._appender is None:
            self._start_appender(k)
        names = self._names()
        while self._appended <= k:                                  # (blocks of a resumed run first, then block k)
            j = self._appended
            self._to_host(j)
            z, th, lp = self.chain[j], self.chain_transformed[j], self.log_prob[j]
            self._appender.append({names[0]: z, names[1]: th, names[2]: lp})
            self._appended += 1
            if z.nbytes >= self.DROP_BYTES:
                # a big block that is in the file does not stay in host memory as well (at 4096 walkers the chain grows
                # by 1.1 MB per iteration): only its length remains here, readers go to the file; its pinned buffers
                # return to the allocator for the next block
                self.chain[j] = self.chain_transformed[j] = self.log_prob[j] = _OnDisk(len(z))
        if self.layout != "zeus":
            self._appender.set_attr("mcmc", "iteration", self._appender.nrows(names[0]))
            if accepted is not None:
                self._appender.set_data("mcmc/accepted", self._acc_host(accepted))

    def arrays(self):
        self.drain()
        for k in range(len(self.chain)):
            self._to_host(k)
        if any(isinstance(b, _OnDisk) for b in self.chain):     # written blocks were dropped: the file has them (and
            if self._appender is not None:                      # whatever is not in it yet goes there first)
                if len(self.chain) > self._appended:
                    self._append_block(len(self.chain) - 1, None)
                self._appender.fh.flush()
            d = self.read_h5(self.h5)
            return d["chain"], d["chain_transformed"], d["log_prob"]
        return (np.concatenate(self.chain), np.concatenate(self.chain_transformed), np.concatenate(self.log_prob))

    def flush(self, final=True):
        """``final=False`` (the incremental flush after every convergence check, sampler.py:359/720): the blocks that
        are not on disk yet are appended to ``<name>.h5`` by the writer thread, one chunk per dataset and block, as the
        reference's HDF5 backend does -- the file is current after every flush and a killed run resumes from it.
        ``final=True``: whatever is left, then the file is closed (a store that was never flushed incrementally writes
        contiguous datasets in one pass); ``<name>.txt`` on request."""
        if not final:
            for k in range(self._flushed, len(self.chain)):
                self._enqueue(None, (k, self.accepted.clone() if torch.is_tensor(self.accepted) else np.array(self.accepted)))
            self._flushed = len(self.chain)
            return
        self.drain()
        for k in range(len(self.chain)):
            self._to_host(k)
        self.accepted = self._acc_host(self.accepted) if self.accepted is not None else None
        if self._appender is not None:                      # the file has grown with the run: add what is left, done
            if len(self.chain) > self._appended:
                self._append_block(len(self.chain) - 1, self.accepted)
            self._appender.close()
            self._appender = None
        else:
            # never flushed incrementally: the blocks go to the file one after the other (contiguous datasets), without a
            # concatenated copy of the chain in memory
            self.write_h5(self.h5, list(self.chain), list(self.chain_transformed), list(self.log_prob), self.accepted, self.layout)
        if self.write_txt:
            z, th, lp = self.arrays()
            flat = np.concatenate([th.reshape(-1, th.shape[-1]), lp.reshape(-1, 1)], axis=1)
            np.savetxt(self.base + ".txt", flat[-100000:])
        for f in self._parts(self.base) + [self.npz]:       # superseded by the consolidated file
            if os.path.isfile(f):
                os.remove(f)
        self._flushed = len(self.chain)

    @staticmethod
    def write_h5(path, z, th, lp, accepted, layout="emcee"):
        w = h5lite.Writer()
        nbytes = lambda a: sum(b.nbytes for b in a) if isinstance(a, list) else a.nbytes
        first = z[0] if isinstance(z, list) else z
        nsteps = sum(len(b) for b in z) if isinstance(z, list) else len(z)
        if layout == "zeus":
            for name, a in (("samples", z), ("chain_transformed", th), ("logprob", lp)):
                w.dataset(None, name, a, compression="gzip" if nbytes(a) <= ChainStore.GZIP_LIMIT else None)
        else:
            nw, nd = first.shape[1], first.shape[2]
            g = w.group("mcmc", attrs=dict(version="3.0.2",                  # the emcee release whose layout this is
                                           nwalkers=np.int64(nw), ndim=np.int64(nd), has_blobs=False,
                                           iteration=np.int64(nsteps)))
            w.dataset(g, "accepted", np.zeros(nw) if accepted is None else np.asarray(accepted, np.float64))
            w.dataset(g, "chain", z)
            w.dataset(g, "chain_transformed", th)
            w.dataset(g, "log_prob", lp)
        tmp = path + ".tmp"
        w.save(tmp)
        os.replace(tmp, path)

    @staticmethod
    def read_h5(path):
        """Either layout, written here or by the reference (h5py)."""
        with h5lite.File(path) as f:
            if "mcmc" in f:
                g = f["mcmc"]
                n = int(g.attrs["iteration"])
                out = {"chain": g["chain"].read(nrows=n), "log_prob": g["log_prob"].read(nrows=n),
                       "accepted": g["accepted"].read()}
                out["chain_transformed"] = g["chain_transformed"].read(nrows=n) if "chain_transformed" in g else None
            else:
                out = {"chain": f["samples"].read(), "chain_transformed": f["chain_transformed"].read(),
                       "log_prob": f["logprob"].read()}
                out["accepted"] = np.zeros(out["chain"].shape[1])
            out["iteration"] = len(out["chain"])
            return out

    def _part(self, k):
        return "%s.part%05d.npz" % (self.base, k)

    @staticmethod
    def _parts(base):
        import glob
        return sorted(glob.glob(base + ".part*.npz"))

    @staticmethod
    def _load_consolidated(base):
        if os.path.isfile(base + ".h5"):
            return ChainStore.read_h5(base + ".h5")
        if os.path.isfile(base + ".npz"):
            d = np.load(base + ".npz")
            return {k: d[k] for k in d.files}
        return None

    @staticmethod
    def load(filename):
        base = filename[:-3] if filename.endswith(".h5") else filename
        parts = ChainStore._parts(base)
        d = ChainStore._load_consolidated(base)
        if parts:                                           # an interrupted run: (consolidated file, if any) + parts
            blocks = [np.load(f) for f in parts]
            out = {k: np.concatenate([b[k] for b in blocks]) for k in ("chain", "chain_transformed", "log_prob")}
            out["accepted"] = blocks[-1]["accepted"]
            if d is not None:
                for k in ("chain", "chain_transformed", "log_prob"):
                    out[k] = np.concatenate([d[k], out[k]])
            out["iteration"] = len(out["chain"])
            return out
        if d is None:
            raise FileNotFoundError(base + ".h5")
        return d

    def get_last_sample(self):
        self.drain()
        return self.load(self.base)["chain"][-1]


def get_good_walker_list(log_prob_samples):
    """util.py:57-66 (``walkercut=True``; no caller in the reference passes it): the walkers whose mean log-probability over
    the last 10000 steps, truncated to an integer, falls into the highest of sklearn's ``KMeans()`` clusters (8 clusters,
    unseeded, as there; ``np.int`` of the reference's numpy is today's ``int``)."""
    from sklearn.cluster import KMeans
    x = np.mean(log_prob_samples[-10000:, :], axis=0)
    X = np.array(list(zip(x, np.zeros(len(x)))), dtype=int)
    ms = KMeans()
    ms.fit(X)
    best = ms.labels_[np.argmax(ms.cluster_centers_[:, 0])]
    print(np.where(ms.labels_ == best)[0], ms.cluster_centers_, ms.labels_)
    return np.where(ms.labels_ == best)[0]


def read_chain_and_cut(chainname, nk, ntimes=20, walkercut=False, method="emcee", flat=False):
    """util.py:68-94: last ``nk`` autocorrelation times of the stored chain (theta space)."""
    d = ChainStore.load(chainname)
    if nk > ntimes:
        print("Error: keep number greater then chain samples. nk: {0}, ntimes: {1}. This will lead to inclusion of all "
              "burn in step".format(nk, ntimes))
    if torch.cuda.is_available():                   # the same estimator, batched on the device (see DeviceChain)
        dc = DeviceChain()
        dc.append(np.asarray(d["chain"], np.float32))
        tau = dc.integrated_time(all_walkers=True)              # util.py:78-80 uses every walker; a one-shot call
    else:
        tau = integrated_time(d["chain"])
    nkeep = int(np.nanmedian(tau) * nk)
    chain = d["chain_transformed"]
    lp = d["log_prob"]
    good = get_good_walker_list(np.asarray(lp)) if walkercut else slice(None)       # util.py:86-89
    chain = np.asarray(chain[-nkeep:][:, good].reshape(-1, chain.shape[-1]), np.float64)
    lp = np.asarray(lp[-nkeep:][:, good], np.float64)
    if flat:
        lp = lp.reshape(-1, 1)
    return chain, lp, d
