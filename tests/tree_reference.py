"""CPU restatements of what the reference's stack walk (trace.metal:144-176) does on a Box[] tree, shared by the tests."""
import numpy as np


def pending_depths(boxes):
    """Entries on the reference's traversal stack underneath each box when it is popped (left+1 is popped first, its sibling
    waits below it).  Parents come before their children in a Box[] array."""
    left = boxes["left"]
    pending = np.zeros(len(boxes), np.int64)
    for i in np.flatnonzero(boxes["right"] == 0):
        pending[left[i] + 1] = pending[i] + 1
        pending[left[i]] = pending[i]
    return pending
