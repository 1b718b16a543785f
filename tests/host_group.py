"""The in-process communicator of the tests that run several row shards of one filter on one GPU (psmf_comm_init_host):
shared by tests/test_hip_multishard.py and the blocked engine's random-configuration net."""

import threading


class HostGroup:
    """In-process stand-in of a communicator: `nranks` threads, sum in rank order, same bits for everybody."""

    def __init__(self, nranks, timeout=60.0):
        self.n = nranks
        self.slots = [None] * nranks
        self.barrier = threading.Barrier(nranks)
        self.timeout = timeout
        self.calls = [0] * nranks
        self.sizes = []

    def allreduce(self, rank):
        def f(v):
            self.slots[rank] = v
            self.barrier.wait(self.timeout)
            tot = self.slots[0].copy()
            for i in range(1, self.n):
                assert self.slots[i].shape == tot.shape
                tot += self.slots[i]
            if rank == 0:
                self.sizes.append(tot.size)
            self.calls[rank] += 1
            self.barrier.wait(self.timeout)
            return tot
        return f
