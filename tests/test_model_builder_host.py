"""ModelBuilder's bookkeeping of a per-vertex policy table, without a GPU: a stand-in context on
the CPU records what the builder hands to the engine (``sl_model_set``, ``sl_policy_touch``)."""

import numpy as np
import torch

from safe_learning_amd import GridWorld, LinearSystem, QuadraticFunction
from safe_learning_amd._model import ModelBuilder


class _Context(object):
    torch_device = torch.device("cpu")

    def __init__(self):
        self.tables, self.touches = [], 0

    def model_set(self, desc):
        self.tables.append(desc.policy.d_table)

    def policy_touch(self):
        self.touches += 1


def _builder():
    grid = GridWorld([[-1., 1.], [-1., 1.]], [4, 5])
    ctx = _Context()
    builder = ModelBuilder(ctx, grid)

    def upload(policy):
        builder.upload(policy, LinearSystem((np.eye(2), np.ones((2, 1)))), QuadraticFunction(np.eye(2)))
    return builder, ctx, grid, upload


def test_in_place_edit_of_a_tensor_policy_is_announced_once():
    _, ctx, grid, upload = _builder()
    table = torch.linspace(-1, 1, grid.nindex, dtype=torch.float64)[:, None].contiguous()
    upload(table)
    upload(table)
    assert ctx.touches == 0                      # the same tensor, unchanged: nothing to announce
    assert ctx.tables == [table.data_ptr()] * 2  # the engine reads the tensor itself
    table[3] = 0.25
    upload(table)
    assert ctx.touches == 1
    upload(table)
    upload(table)
    assert ctx.touches == 1
    table.copy_(-table)
    table.view(-1)[7] = 0.5                      # (a view shares the version counter)
    upload(table)
    assert ctx.touches == 2
    assert ctx.tables[-1] == table.data_ptr()


def test_a_one_dimensional_tensor_policy_is_followed_too():
    _, ctx, grid, upload = _builder()
    table = torch.zeros(grid.nindex, dtype=torch.float64)
    upload(table)
    table[0] = 1.0
    upload(table)
    assert ctx.touches == 1 and ctx.tables == [table.data_ptr()] * 2


def test_another_view_of_the_same_storage_is_announced():
    """Whatever was written through an alias, the engine cannot tell: a new tensor object on the
    storage it reads is announced."""
    _, ctx, grid, upload = _builder()
    table = torch.zeros((grid.nindex, 1), dtype=torch.float64)
    upload(table)
    upload(table.view(-1))
    assert ctx.touches == 1 and ctx.tables == [table.data_ptr()] * 2


def test_a_new_tensor_changes_the_descriptor_instead():
    builder, ctx, grid, upload = _builder()
    first = torch.zeros((grid.nindex, 1), dtype=torch.float64)
    upload(first)
    second = torch.ones((grid.nindex, 1), dtype=torch.float64)
    upload(second)
    assert ctx.touches == 0
    assert ctx.tables == [first.data_ptr(), second.data_ptr()] and ctx.tables[0] != ctx.tables[1]
    # the builder holds the table the engine points at
    assert builder._policy_table.data_ptr() == second.data_ptr()


def test_copied_policy_tables_need_no_announcement():
    """A NumPy array or a float32 tensor is copied at every upload: each copy is a new table."""
    builder, ctx, grid, upload = _builder()
    array = np.zeros((grid.nindex, 1))
    upload(array)
    array[2] = 1.0
    upload(array)
    single = torch.zeros((grid.nindex, 1), dtype=torch.float32)
    upload(single)
    single[2] = 1.0
    upload(single)
    assert ctx.touches == 0
    assert builder._policy_table.dtype == torch.float64
    assert float(builder._policy_table[2, 0]) == 1.0
