"""CPU: what the pipelines' batch_decode argument resolves to (driver.resolve_batch_decode, a pure function)."""
import pytest

from samrs_amd import driver

# (batch_decode, batch, box_batch, max_boxes, max_prompts, max_images, capacity) -> (on, decode_prompts to set)
TABLE = [
    # the c2 shape of the benchmark: 8 tiles x 32 boxes, engine created for 32-prompt predicts on 16 slots
    (("auto", 8, 32, 32, 32, 16, 32), (True, 256)),
    # c4: the same shape at another box count; box_batch above max_boxes changes nothing (a chain holds batch x max_boxes)
    (("auto", 8, 16, 16, 16, 16, 16), (True, 128)),
    (("auto", 8, 64, 32, 32, 16, 32), (True, 256)),
    # c3: long-tailed tiles decoded in several chunks stay per tile
    (("auto", 8, 64, 400, 64, 16, 64), (False, None)),
    (("auto", 2, 3, 8, 64, 4, 64), (False, None)),
    # the capacity is there already (a roomy max_prompts, or an earlier pipeline raised it): on, nothing to set
    (("auto", 2, 3, 3, 64, 4, 64), (True, None)),
    (("auto", 2, 3, 3, 3, 4, 6), (True, None)),
    (("auto", 2, 3, 3, 3, 4, 3), (True, 6)),
    # beyond what the engine accepts: max_images x max_prompts, and the 512 the index types carry
    (("auto", 4, 3, 3, 3, 3, 3), (False, None)),
    (("auto", 8, 32, 32, 32, 16, 256), (True, None)),
    (("auto", 16, 64, 64, 64, 32, 64), (False, None)),
    (("auto", 8, 64, 64, 64, 16, 64), (True, 512)),
    # True / False keep their meaning and never ask for anything
    ((True, 8, 64, 400, 64, 16, 64), (True, None)),
    ((False, 8, 32, 32, 32, 16, 32), (False, None)),
    ((1, 2, 3, 8, 64, 4, 64), (True, None)),
    ((0, 8, 32, 32, 32, 16, 32), (False, None)),
]


@pytest.mark.parametrize("args,expected", TABLE)
def test_resolution_rule(args, expected):
    on, want, why = driver.resolve_batch_decode(*args)
    assert (on, want) == expected, why
    assert isinstance(why, str) and why
    if want is not None:                                    # only ever a value the engine's documented range admits
        _, batch, _, max_boxes, max_prompts, max_images, capacity = args
        assert capacity < want == batch * max_boxes and max_prompts <= want <= min(max_images * max_prompts, driver.DECODE_PROMPTS_LIMIT)


def test_default_is_auto():
    import inspect
    assert inspect.signature(driver.TilePipeline.__init__).parameters["batch_decode"].default == "auto"
