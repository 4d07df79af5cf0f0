"""The decode-stream timer the pipeline bench tools share (batch_decode_bench, clean_masks_bench, mask_boxes_bench, quality_bench,
polygons_bench)."""
import torch


def time_decode(pipe) -> list:
    """Wraps `pipe._decode` with two timing events on the decode stream, behind the wait for the encoder that _decode itself
    begins with: the events time the work, not the wait.  Returns the list the (start, end) pairs are appended to, one per
    batch; ``decode_ms(events)`` reads them after a synchronise.  (_decode is a private method of TilePipeline: if its first wait
    changes, this wrapper has to follow.)"""
    events, decode = [], pipe._decode

    def timed(b, its, tiles, offs, out):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        pipe.s_dec.wait_event(pipe.ev_enc[b])          # the decode's own first wait: time the work, not the wait for the encoder
        e0.record(pipe.s_dec)
        decode(b, its, tiles, offs, out)
        e1.record(pipe.s_dec)
        events.append((e0, e1))

    pipe._decode = timed
    return events


def decode_ms(events) -> list:
    return [a.elapsed_time(b) for a, b in events]
