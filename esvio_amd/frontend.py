"""Host-side mirror of the reference's feature_tracker interface over the C ABI.

``FeatureTracker`` / ``EventDetector`` keep the reference's names and argument meaning
(feature_tracker/src/feature_tracker.h:49-173, event_detector/event_detector.h:18-80) so the
parity tests read like calls into the reference.  Everything here is ctypes plumbing over
``libesvio_fe.so`` (include/esvio_fe.h); there is no Python compute path and no CPU fallback —
if the library or a GPU is missing, construction raises.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST, DEVICE = 0, 1
EVENT_IMAGES_AHEAD = 2  # ESVIO_FE_EVENT_IMAGES_AHEAD
LK_USE_INITIAL_FLOW = 4


class FrontendError(RuntimeError):
    pass


class Camera(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")]


class Config(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("decay_ms", C.c_double),
        ("ignore_polarity", C.c_int32), ("median_blur_kernel_size", C.c_int32),
        ("feature_filter_threshold", C.c_double),
        ("ts_lk_threshold", C.c_double),
        ("max_cnt", C.c_int32), ("min_dist", C.c_int32),
        ("flow_back", C.c_int32), ("equalize", C.c_int32),
        ("f_threshold", C.c_double),
        ("f_ransac", C.c_int32), ("lk_accum", C.c_int32),
        ("focal_length", C.c_int32), ("device", C.c_int32),
        ("cam", Camera * 2),
    ]


class Motion(C.Structure):
    """esvio_fe_motion: the Motion_correction_value fields createSAE_* reads + detector.init's K"""
    _fields_ = [("t1", C.c_double), ("v", C.c_double * 3), ("v_pre", C.c_float * 3),
                ("accel", C.c_float * 3), ("omega", C.c_float * 3),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


def make_motion(t1, v, v_pre, accel, omega, fx, fy, cx, cy):
    m = Motion()
    m.t1 = float(t1)
    for i in range(3):
        m.v[i] = float(v[i])
        m.v_pre[i] = float(v_pre[i])
        m.accel[i] = float(accel[i])
        m.omega[i] = float(omega[i])
    m.fx, m.fy, m.cx, m.cy = float(fx), float(fy), float(cx), float(cy)
    return m


class EventFieldsDesc(C.Structure):
    """esvio_fe_event_fields"""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("t", C.c_void_p), ("p", C.c_void_p),
                ("x_stride", C.c_int32), ("y_stride", C.c_int32), ("t_stride", C.c_int32), ("p_stride", C.c_int32),
                ("t_bits", C.c_int32), ("t_unit_ns", C.c_int32), ("p_bits", C.c_int32), ("t_offset", C.c_int64)]


def fields_desc(f):
    """events.EventFields -> esvio_fe_event_fields"""
    d = EventFieldsDesc()
    d.x, d.y, d.t, d.p = f.ptrs
    d.x_stride, d.y_stride, d.t_stride, d.p_stride = f.strides
    d.t_bits, d.t_unit_ns, d.p_bits, d.t_offset = f.t_bits, f.t_unit_ns, f.p_bits, f.t_offset
    return d


class FilterParams(C.Structure):
    """esvio_fe_filter_params (include/esvio_fe.h has the rule): min_support 0 skips the support test, refractory_ns 0
    the refractory test"""
    _fields_ = [("window_ns", C.c_int64), ("min_support", C.c_int32), ("reserved", C.c_int32), ("refractory_ns", C.c_int64)]

    def __init__(self, window_ns=0, min_support=1, refractory_ns=0):
        super().__init__(int(window_ns), int(min_support), 0, int(refractory_ns))


class AddressFilter(C.Structure):
    """esvio_fe_address_filter (include/esvio_fe.h: step 1a of the filter rule): roi = (x0, y0, x1, y1), inclusive;
    polarity 0 both / 1 ON only / 2 OFF only; flatten 0 / 1 / 2; use_mask: reject the camera's masked pixels"""
    _fields_ = [("roi_x0", C.c_uint16), ("roi_y0", C.c_uint16), ("roi_x1", C.c_uint16), ("roi_y1", C.c_uint16),
                ("polarity", C.c_int32), ("flatten", C.c_int32), ("use_mask", C.c_int32), ("reserved", C.c_int32)]

    def __init__(self, roi=(0, 0, 0, 0), polarity=0, flatten=0, use_mask=0):
        super().__init__(int(roi[0]), int(roi[1]), int(roi[2]), int(roi[3]), int(polarity), int(flatten), int(use_mask), 0)


class HotParams(C.Structure):
    """esvio_fe_hot_params"""
    _fields_ = [("max_pixels", C.c_uint32), ("min_count", C.c_uint32), ("min_rate_hz", C.c_uint32), ("mean_factor", C.c_uint32),
                ("install", C.c_int32), ("reserved", C.c_int32)]

    def __init__(self, max_pixels=8, min_count=1, min_rate_hz=0, mean_factor=0, install=False):
        super().__init__(int(max_pixels), int(min_count), int(min_rate_hz), int(mean_factor), int(bool(install)), 0)


class HotInfo(C.Structure):
    """esvio_fe_hot_info"""
    _fields_ = [("events", C.c_uint64), ("span_ns", C.c_uint64), ("threshold", C.c_uint64), ("above", C.c_uint32),
                ("selected", C.c_uint32)]


class Batch(C.Structure):
    """esvio_fe_batch"""
    _fields_ = [("left", C.c_void_p), ("right", C.c_void_p), ("left_fields", C.POINTER(EventFieldsDesc)),
                ("right_fields", C.POINTER(EventFieldsDesc)), ("nL", C.c_size_t), ("nR", C.c_size_t), ("space", C.c_int32),
                ("pub_this_frame", C.c_int32), ("filter", C.POINTER(FilterParams)), ("motion", C.POINTER(Motion)),
                ("cur_time", C.c_double), ("cur_time_from_batch", C.c_int32), ("reserved", C.c_int32)]


class BatchInfo(C.Structure):
    """esvio_fe_batch_info"""
    _fields_ = [("kept", C.c_uint64 * 2), ("rejected", C.c_uint64 * 2), ("bad", C.c_uint64 * 2), ("cur_time", C.c_double),
                ("tracked", C.c_int32), ("reserved", C.c_int32)]


class RawInfo(C.Structure):
    """esvio_fe_raw_info"""
    _fields_ = [("events", C.c_uint64), ("untimed", C.c_uint64), ("other", C.c_uint64), ("bad", C.c_uint64),
                ("wraps", C.c_uint64), ("first_t_us", C.c_int64), ("last_t_us", C.c_int64)]


RAW_EVT2, RAW_EVT3, RAW_EVT21 = 2, 3, 21  # esvio_fe_decode_raw's formats
RAW_WORD_BYTES = {RAW_EVT2: 4, RAW_EVT3: 2, RAW_EVT21: 8}


def raw_bound(fmt, nbytes):
    """the records nbytes of words of format fmt can stand for at most (include/esvio_fe.h)"""
    return nbytes // 2 * 12 if fmt == RAW_EVT3 else nbytes * 4 if fmt == RAW_EVT21 else nbytes // 4


class TextFormat(C.Structure):
    """esvio_fe_text_format"""
    _fields_ = [("order", C.c_int32), ("time", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class TextInfo(C.Structure):
    """esvio_fe_text_info"""
    _fields_ = [("events", C.c_uint64), ("lines", C.c_uint64), ("comments", C.c_uint64), ("blank", C.c_uint64),
                ("malformed", C.c_uint64), ("bad", C.c_uint64), ("first_malformed", C.c_int64), ("first_t_ns", C.c_int64),
                ("last_t_ns", C.c_int64), ("carried", C.c_uint32), ("reserved", C.c_uint32)]


class TextLimits(C.Structure):
    """esvio_fe_text_limits_info (include/esvio_fe_test.h)"""
    _fields_ = [("tile_bytes", C.c_int32), ("max_body", C.c_int32), ("max_tail", C.c_int32), ("reserved", C.c_int32)]


class ScanLanes(C.Structure):
    """esvio_fe_scan_lanes_info (include/esvio_fe_test.h)"""
    _fields_ = [("raw", C.c_int32), ("aedat", C.c_int32), ("text", C.c_int32), ("slice", C.c_int32), ("filter", C.c_int32),
                ("pick", C.c_int32), ("filter_block_events", C.c_int32), ("pick_tile_values", C.c_int32)]


TEXT_TXYP, TEXT_XYPT = 1, 2                          # esvio_fe_text_format.order
TEXT_SEC_DECIMAL, TEXT_INT_US, TEXT_INT_NS = 1, 2, 3  # .time
TEXT_END, TEXT_SKIP_MALFORMED = 1, 2                  # .flags


def text_bound(nbytes):
    """the records a text chunk of nbytes can hold at the most, whatever tail is carried (include/esvio_fe.h)"""
    return (nbytes + 65) // 8 + 1


def _text_src(data):
    """(pointer, n_bytes, space, keep-alive) of a text chunk: bytes, a contiguous numpy array or a (device_ptr, n_bytes) tuple"""
    if isinstance(data, tuple):
        return C.c_void_p(data[0]), int(data[1]), DEVICE, None
    buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data)
    return (_p(buf) if buf.nbytes else None), buf.nbytes, HOST, buf


class Trigger(C.Structure):
    """esvio_fe_trigger"""
    _fields_ = [("sec", C.c_uint32), ("nsec", C.c_uint32), ("id", C.c_uint8), ("value", C.c_uint8), ("_pad", C.c_uint8 * 6)]


TRIGGER_DTYPE = np.dtype([("sec", "<u4"), ("nsec", "<u4"), ("id", "u1"), ("value", "u1"), ("_pad", "u1", (6,))])


class TriggerInfo(C.Structure):
    """esvio_fe_trigger_info"""
    _fields_ = [("triggers", C.c_uint64), ("untimed", C.c_uint64), ("bad", C.c_uint64), ("wraps", C.c_uint64),
                ("first_t_us", C.c_int64), ("last_t_us", C.c_int64)]


class RawHeaderInfo(C.Structure):
    """esvio_fe_raw_header_info"""
    _fields_ = [("payload_offset", C.c_uint64), ("format", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("complete", C.c_int32)]


AEDAT_KEEP_INVALID = 1  # ESVIO_FE_AEDAT_KEEP_INVALID


class AedatInfo(C.Structure):
    """esvio_fe_aedat_info"""
    _fields_ = [("events", C.c_uint64), ("invalid", C.c_uint64), ("bad", C.c_uint64), ("polarity_packets", C.c_uint64),
                ("other_packets", C.c_uint64), ("first_t_us", C.c_int64), ("last_t_us", C.c_int64)]


class ImuSample(C.Structure):
    """esvio_fe_imu_sample"""
    _fields_ = [("sec", C.c_uint32), ("nsec", C.c_uint32), ("acc", C.c_double * 3), ("gyr", C.c_double * 3)]


IMU_DTYPE = np.dtype([("sec", "<u4"), ("nsec", "<u4"), ("acc", "<f8", (3,)), ("gyr", "<f8", (3,))])


class AedatSideInfo(C.Structure):
    """esvio_fe_aedat_side_info"""
    _fields_ = [("imu", C.c_uint64), ("triggers", C.c_uint64), ("resets", C.c_uint64), ("other_specials", C.c_uint64),
                ("invalid", C.c_uint64), ("bad", C.c_uint64), ("special_packets", C.c_uint64), ("imu_packets", C.c_uint64),
                ("other_packets", C.c_uint64)]


class AedatHeaderInfo(C.Structure):
    """esvio_fe_aedat_header_info"""
    _fields_ = [("payload_offset", C.c_uint64), ("version", C.c_int32), ("complete", C.c_int32)]


class AedatFrame(C.Structure):
    """esvio_fe_aedat_frame"""
    _fields_ = [("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32), ("ts_startframe", C.c_int32), ("ts_endframe", C.c_int32),
                ("ts_startexposure", C.c_int32), ("ts_endexposure", C.c_int32), ("exposure_us", C.c_int64), ("length_x", C.c_int32),
                ("length_y", C.c_int32), ("position_x", C.c_int32), ("position_y", C.c_int32), ("channels", C.c_int32),
                ("color_filter", C.c_int32), ("roi", C.c_int32), ("valid", C.c_int32), ("slot", C.c_int32), ("ts_overflow", C.c_int32),
                ("index", C.c_uint64)]


AEDAT_FRAME_DTYPE = np.dtype([("stamp_sec", "<u4"), ("stamp_nsec", "<u4"), ("ts_startframe", "<i4"), ("ts_endframe", "<i4"),
                              ("ts_startexposure", "<i4"), ("ts_endexposure", "<i4"), ("exposure_us", "<i8"), ("length_x", "<i4"),
                              ("length_y", "<i4"), ("position_x", "<i4"), ("position_y", "<i4"), ("channels", "<i4"),
                              ("color_filter", "<i4"), ("roi", "<i4"), ("valid", "<i4"), ("slot", "<i4"), ("ts_overflow", "<i4"),
                              ("index", "<u8")])


class AedatFrameInfo(C.Structure):
    """esvio_fe_aedat_frame_info"""
    _fields_ = [("frames", C.c_uint64), ("invalid", C.c_uint64), ("bad", C.c_uint64), ("frame_packets", C.c_uint64),
                ("other_packets", C.c_uint64), ("first_sec", C.c_uint32), ("first_nsec", C.c_uint32), ("last_sec", C.c_uint32),
                ("last_nsec", C.c_uint32)]


class BagTopics(C.Structure):
    """esvio_fe_bag_topics"""
    _fields_ = [("left", C.c_char_p), ("right", C.c_char_p), ("imu", C.c_char_p)]


class BagHeaderInfo(C.Structure):
    """esvio_fe_bag_header_info"""
    _fields_ = [("payload_offset", C.c_uint64), ("index_pos", C.c_uint64), ("conn_count", C.c_uint32), ("chunk_count", C.c_uint32),
                ("version", C.c_int32), ("complete", C.c_int32)]


class BagMessage(C.Structure):
    """esvio_fe_bag_message"""
    _fields_ = [("cam", C.c_int32), ("seq", C.c_uint32), ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32), ("time_sec", C.c_uint32),
                ("time_nsec", C.c_uint32), ("height", C.c_uint32), ("width", C.c_uint32), ("first", C.c_uint64), ("count", C.c_uint64)]


BAG_MESSAGE_DTYPE = np.dtype([("cam", "<i4"), ("seq", "<u4"), ("stamp_sec", "<u4"), ("stamp_nsec", "<u4"), ("time_sec", "<u4"),
                              ("time_nsec", "<u4"), ("height", "<u4"), ("width", "<u4"), ("first", "<u8"), ("count", "<u8")])


class BagCamInfo(C.Structure):
    """esvio_fe_bag_cam_info"""
    _fields_ = [("events", C.c_uint64), ("bad", C.c_uint64), ("messages", C.c_uint64), ("first_sec", C.c_uint32), ("first_nsec", C.c_uint32),
                ("last_sec", C.c_uint32), ("last_nsec", C.c_uint32)]


class BagInfo(C.Structure):
    """esvio_fe_bag_info"""
    _fields_ = [("cam", BagCamInfo * 2), ("other_messages", C.c_uint64), ("other_records", C.c_uint64), ("chunks", C.c_uint64),
                ("connections", C.c_uint64)]


class BagSideInfo(C.Structure):
    """esvio_fe_bag_side_info"""
    _fields_ = [("imu", C.c_uint64), ("bad", C.c_uint64), ("other_messages", C.c_uint64), ("other_records", C.c_uint64),
                ("chunks", C.c_uint64), ("connections", C.c_uint64)]


class BagImage(C.Structure):
    """esvio_fe_bag_image"""
    _fields_ = [("cam", C.c_int32), ("seq", C.c_uint32), ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32), ("time_sec", C.c_uint32),
                ("time_nsec", C.c_uint32), ("height", C.c_uint32), ("width", C.c_uint32), ("step", C.c_uint32), ("encoding", C.c_int32),
                ("is_bigendian", C.c_int32), ("index", C.c_uint64)]


BAG_IMAGE_DTYPE = np.dtype({"names": ["cam", "seq", "stamp_sec", "stamp_nsec", "time_sec", "time_nsec", "height", "width", "step", "encoding",
                                      "is_bigendian", "index"],
                            "formats": ["<i4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<i4", "<i4", "<u8"],
                            "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 48], "itemsize": 56})
ENC_MONO, ENC_BGR, ENC_RGB = 1, 2, 3  # esvio_fe_bag_image.encoding: mono8 | 8UC1, bgr8 | 8UC3, rgb8


class BagImageCamInfo(C.Structure):
    """esvio_fe_bag_image_cam_info"""
    _fields_ = [("images", C.c_uint64), ("first_sec", C.c_uint32), ("first_nsec", C.c_uint32), ("last_sec", C.c_uint32), ("last_nsec", C.c_uint32)]


class BagImageInfo(C.Structure):
    """esvio_fe_bag_image_info"""
    _fields_ = [("cam", BagImageCamInfo * 2), ("other_messages", C.c_uint64), ("other_records", C.c_uint64), ("chunks", C.c_uint64),
                ("connections", C.c_uint64)]


class EventRecord(C.Structure):
    """esvio_fe_event"""
    _fields_ = [("x", C.c_uint16), ("y", C.c_uint16), ("sec", C.c_uint32), ("nsec", C.c_uint32), ("polarity", C.c_uint8),
                ("_pad", C.c_uint8 * 3)]


class SliceParams(C.Structure):
    """esvio_fe_slice_params (include/esvio_fe.h has the rule): origin None: the camera's first event; else (sec, nsec)"""
    _fields_ = [("frequency", C.c_double), ("origin", EventRecord), ("has_origin", C.c_int32), ("reserved", C.c_int32)]

    def __init__(self, frequency=30.0, origin=None):
        super().__init__(float(frequency))
        if origin is not None:
            self.origin.sec, self.origin.nsec, self.has_origin = int(origin[0]), int(origin[1]), 1


class SliceInfo(C.Structure):
    """esvio_fe_slice_info"""
    _fields_ = [("closed", C.c_uint64), ("first_window", C.c_uint64), ("count", C.c_uint64), ("open_events", C.c_uint64),
                ("first_sec", C.c_uint32), ("first_nsec", C.c_uint32), ("last_sec", C.c_uint32), ("last_nsec", C.c_uint32)]


SLICE_MAX_WINDOWS = 4096  # ESVIO_FE_SLICE_MAX_WINDOWS


class FeedInfo(C.Structure):
    """esvio_fe_feed_info"""
    _fields_ = [("appended", C.c_uint64), ("rejected", C.c_uint64), ("bad", C.c_uint64), ("closed", C.c_uint64),
                ("queued", C.c_uint64)]


class FeedWindow(C.Structure):
    """esvio_fe_feed_window"""
    _fields_ = [("ready", C.c_int32), ("reserved", C.c_int32), ("index", C.c_uint64), ("end_sec", C.c_uint32),
                ("end_nsec", C.c_uint32), ("count", C.c_uint64 * 2)]


class Tracks(C.Structure):
    _fields_ = [
        ("n_left", C.c_int32), ("n_right", C.c_int32),
        ("ids", C.c_void_p), ("track_cnt", C.c_void_p),
        ("cur_pts", C.c_void_p), ("cur_un_pts", C.c_void_p), ("pts_velocity", C.c_void_p),
        ("ids_right", C.c_void_p), ("cur_right_pts", C.c_void_p),
        ("cur_un_right_pts", C.c_void_p), ("right_pts_velocity", C.c_void_p),
    ]


# every symbol include/esvio_fe.h declares
# the drop-in boundary: every entry point include/esvio_fe.h declares (INTEGRATION.md section 3 maps each to the
# reference call it replaces)
ABI_SYMBOLS = [
    "esvio_fe_calc_optical_flow_pyr_lk", "esvio_fe_comm_init", "esvio_fe_comm_unique_id",
    "esvio_fe_convert_events", "esvio_fe_create", "esvio_fe_decode_raw", "esvio_fe_decode_reset",
    "esvio_fe_decode_triggers", "esvio_fe_raw_header", "esvio_fe_slice_events_at",
    "esvio_fe_aedat_header", "esvio_fe_decode_aedat", "esvio_fe_aedat_side", "esvio_fe_track_aedat", "esvio_fe_feed_push_aedat",
    "esvio_fe_decode_aedat_frames", "esvio_fe_convert_frame16",
    "esvio_fe_bag_header", "esvio_fe_bag_set_topics", "esvio_fe_decode_bag", "esvio_fe_bag_side", "esvio_fe_feed_push_bag",
    "esvio_fe_bag_set_image_topics", "esvio_fe_decode_bag_images", "esvio_fe_convert_image", "esvio_fe_track_image_space",
    "esvio_fe_create_sae", "esvio_fe_create_sae_stereo", "esvio_fe_create_sae_stereo_mc", "esvio_fe_destroy",
    "esvio_fe_exchange_begin", "esvio_fe_exchange_end", "esvio_fe_exchange_tracks", "esvio_fe_export_image",
    "esvio_fe_feed_close", "esvio_fe_feed_open", "esvio_fe_feed_peek", "esvio_fe_feed_push_events", "esvio_fe_feed_push_fields",
    "esvio_fe_feed_push_raw", "esvio_fe_feed_track",
    "esvio_fe_fast_corners", "esvio_fe_filter_batch", "esvio_fe_filter_events", "esvio_fe_filter_reset", "esvio_fe_features_to_track", "esvio_fe_features_to_track_fast", "esvio_fe_find_fundamental_mat", "esvio_fe_finish", "esvio_fe_get_sae",
    "esvio_fe_get_pixel_mask", "esvio_fe_get_time_surface", "esvio_fe_good_features_to_track", "esvio_fe_hot_learn",
    "esvio_fe_hot_reset", "esvio_fe_hot_select", "esvio_fe_import_image", "esvio_fe_is_corner",
    "esvio_fe_last_error", "esvio_fe_mem_alloc", "esvio_fe_mem_free", "esvio_fe_mem_upload",
    "esvio_fe_pack_track_records", "esvio_fe_register_host_buffer", "esvio_fe_reserve", "esvio_fe_reset",
    "esvio_fe_sae_plane_doubles", "esvio_fe_sae_slice_apply", "esvio_fe_sae_slice_commit",
    "esvio_fe_sae_slice_last", "esvio_fe_sae_to_time_surface", "esvio_fe_set_address_filter", "esvio_fe_set_auto_exchange",
    "esvio_fe_set_detector", "esvio_fe_set_pixel_mask",
    "esvio_fe_set_event_images", "esvio_fe_clear_event_images", "esvio_fe_get_event_image", "esvio_fe_get_event_canvas",
    "esvio_fe_set_host_threads", "esvio_fe_set_launch_thread", "esvio_fe_set_lazy_new_stereo",
    "esvio_fe_set_next_batch", "esvio_fe_set_next_batch_mc", "esvio_fe_slice_events", "esvio_fe_slice_flush",
    "esvio_fe_slice_reset", "esvio_fe_track_batch", "esvio_fe_track_event", "esvio_fe_track_event_fields",
    "esvio_fe_track_event_filtered", "esvio_fe_track_event_mc", "esvio_fe_track_raw",
    "esvio_fe_track_image", "esvio_fe_unregister_host_buffer", "esvio_fe_version",
    "esvio_fe_kf_set_pattern", "esvio_fe_kf_blur", "esvio_fe_kf_fast", "esvio_fe_kf_brief", "esvio_fe_kf_match",
    "esvio_fe_kf_describe",
    "esvio_fe_bow_vocabulary_header", "esvio_fe_bow_set_vocabulary", "esvio_fe_bow_transform", "esvio_fe_bow_add",
    "esvio_fe_bow_query", "esvio_fe_bow_detect_loop", "esvio_fe_bow_clear", "esvio_fe_bow_entries", "esvio_fe_bow_reserve",
    "esvio_fe_bow_create_vocabulary", "esvio_fe_bow_get_created",
    "esvio_fe_decode_text", "esvio_fe_track_text", "esvio_fe_feed_push_text", "esvio_fe_text_imu", "esvio_fe_text_images",
]
# test / measurement taps: include/esvio_fe_test.h (not part of the boundary)
TEST_SYMBOLS = [
    "esvio_fe_build_pyramid", "esvio_fe_debug_counters", "esvio_fe_debug_inject", "esvio_fe_device_memory",
    "esvio_fe_export_level",
    "esvio_fe_find_fundamental_mat_held", "esvio_fe_find_fundamental_mat_idle", "esvio_fe_find_fundamental_mat_mt",
    "esvio_fe_get_kernel_stats", "esvio_fe_host_hypot", "esvio_fe_host_nullspace", "esvio_fe_host_stage_copy",
    "esvio_fe_host_stage_pack", "esvio_fe_staging_counters",
    "esvio_fe_kernel_count", "esvio_fe_kernel_name", "esvio_fe_latency_phase_name", "esvio_fe_latency_recent",
    "esvio_fe_latency_stats", "esvio_fe_lift_projective", "esvio_fe_plain_call_counters", "esvio_fe_ransac_stats",
    "esvio_fe_ransac_tail", "esvio_fe_raw_tile_bytes", "esvio_fe_reset_kernel_stats", "esvio_fe_select_candidates",
    "esvio_fe_set_profiling", "esvio_fe_set_sae",
    "esvio_fe_slice_tile_events", "esvio_fe_stage_kernel_count", "esvio_fe_stream",
    "esvio_fe_aedat_tile_events", "esvio_fe_ingest_kernel_count", "esvio_fe_aedat_walk_tap", "esvio_fe_aedat_walk_state_bytes",
    "esvio_fe_bag_tile_events", "esvio_fe_bag_walk_tap", "esvio_fe_bag_walk_state_bytes",
    "esvio_fe_bag_image_walk_tap", "esvio_fe_image_tile_pixels", "esvio_fe_event_image_kernel_stats",
    "esvio_fe_aedat_frame_walk_tap", "esvio_fe_aedat_frame_kernel_stats", "esvio_fe_frame16_tile_pixels",
    "esvio_fe_kf_kernel_count", "esvio_fe_kf_kernel_name", "esvio_fe_kf_kernel_stats", "esvio_fe_kf_blur_tile",
    "esvio_fe_bow_kernel_count", "esvio_fe_bow_kernel_name", "esvio_fe_bow_kernel_stats", "esvio_fe_bow_limits", "esvio_fe_bow_scores",
    "esvio_fe_bow_create_kernel_count", "esvio_fe_bow_create_kernel_name", "esvio_fe_bow_create_kernel_stats", "esvio_fe_bow_create_pick",
    "esvio_fe_text_limits", "esvio_fe_text_kernel_count", "esvio_fe_text_kernel_name", "esvio_fe_text_kernel_stats",
    "esvio_fe_scan_lanes", "esvio_fe_sort_pairs",
]

LATENCY_PHASES = 16
SELECT_EUCLID, SELECT_TABLE = 1, 2  # esvio_fe_select_candidates' flags (include/esvio_fe_test.h)


class LatencyCall(C.Structure):  # esvio_fe_latency_call
    _fields_ = [("call", C.c_uint64), ("published", C.c_int32), ("reserved", C.c_int32), ("begin_ms", C.c_double),
                ("ms", C.c_double), ("phase_ms", C.c_double * LATENCY_PHASES)]


class KfOut(C.Structure):  # esvio_fe_kf_out
    _fields_ = [("window_desc", C.c_void_p), ("kp_xy", C.c_void_p), ("kp_score", C.c_void_p), ("kp_norm", C.c_void_p),
                ("kp_desc", C.c_void_p), ("kp_capacity", C.c_int32), ("n_kp", C.c_int32), ("n_detected", C.c_int32),
                ("desc_space", C.c_int32)]


KF_BEST_INIT, KF_MATCH_DIST = 128, 80  # ESVIO_FE_KF_BEST_INIT, ESVIO_FE_KF_MATCH_DIST


class BowVocabularyInfo(C.Structure):  # esvio_fe_bow_vocabulary_info
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("scoring", C.c_int32), ("weighting", C.c_int32), ("nodes", C.c_int32),
                ("words", C.c_int32), ("leaves", C.c_int32), ("max_children", C.c_int32), ("depth", C.c_int32),
                ("message", C.c_char * 188)]


class BowResult(C.Structure):  # esvio_fe_bow_result
    _fields_ = [("id", C.c_int32), ("score", C.c_double)]


class BowCreateParams(C.Structure):  # esvio_fe_bow_create_params
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("weighting", C.c_int32), ("scoring", C.c_int32), ("max_passes", C.c_int32),
                ("reserved", C.c_int32), ("seed", C.c_uint64)]


class BowCreateInfo(C.Structure):  # esvio_fe_bow_create_info
    _fields_ = [("nodes", C.c_int32), ("words", C.c_int32), ("depth", C.c_int32), ("max_children", C.c_int32),
                ("kmeans_nodes", C.c_int32), ("passes", C.c_int32), ("empty_clusters", C.c_int32), ("short_seedings", C.c_int32),
                ("bytes", C.c_uint64), ("message", C.c_char * 188)]


class BowLimits(C.Structure):  # esvio_fe_bow_limits_info
    _fields_ = [("group_lanes", C.c_int32), ("lds_words", C.c_int32), ("vector_block", C.c_int32), ("max_results", C.c_int32)]


# ESVIO_FE_BOW_MAX_RESULTS, _LOOP_RESULTS, _LOOP_GAP, _LOOP_MIN_FIRST, _LOOP_MIN_OTHER
BOW_MAX_RESULTS, BOW_LOOP_RESULTS, BOW_LOOP_GAP, BOW_LOOP_MIN_FIRST, BOW_LOOP_MIN_OTHER = 64, 4, 50, 0.05, 0.015


def bow_vocabulary_header(data):
    """esvio_fe_bow_vocabulary_header on a vocabulary file's bytes (no handle, no device) -> (return code, dict of the
    info struct's fields, message as str)"""
    buf = bytes(data)
    info = BowVocabularyInfo()
    rc = load_library().esvio_fe_bow_vocabulary_header(buf, len(buf), C.byref(info))
    d = {n: getattr(info, n) for n, _ in BowVocabularyInfo._fields_ if n != "message"}
    d["message"] = info.message.decode()
    return rc, d


def bow_limits():
    """esvio_fe_bow_limits -> dict"""
    o = BowLimits()
    assert load_library().esvio_fe_bow_limits(C.byref(o)) == 0
    return {n: getattr(o, n) for n, _ in BowLimits._fields_}


def parse_brief_pattern(text):
    """brief_pattern.yml as BriefExtractor reads it (keyframe.cpp:623-640): the four top-level lists x1, y1, x2, y2 of
    the file's list-of-integers YAML (`key:` lines, `- value` items, or one flow list `key: [a, b, ...]`) ->
    (x1, y1, x2, y2) int32 arrays.  Nothing else of YAML is understood; anything else raises ValueError."""
    lists, cur = {}, None
    for ln, raw in enumerate(text.splitlines(), 1):
        line = raw.split("#", 1)[0].strip() if not raw.startswith("%") else ""
        if not line or line == "---":
            continue
        if line.startswith("-"):
            if cur is None:
                raise ValueError("brief pattern, line %d: an item outside a list" % ln)
            lists[cur].append(int(line[1:].strip()))
        elif ":" in line:
            key, rest = line.split(":", 1)
            cur = key.strip()
            lists[cur] = []
            rest = rest.strip()
            if rest:
                if not (rest.startswith("[") and rest.endswith("]")):
                    raise ValueError("brief pattern, line %d: not a list of integers" % ln)
                lists[cur] = [int(v) for v in rest[1:-1].split(",") if v.strip()]
                cur = None
        else:
            raise ValueError("brief pattern, line %d: %r" % (ln, raw))
    try:
        out = tuple(np.array(lists[k], np.int32) for k in ("x1", "y1", "x2", "y2"))
    except KeyError as e:
        raise ValueError("brief pattern: list %s is missing" % e)
    if len({len(a) for a in out}) != 1:
        raise ValueError("brief pattern: the four lists differ in length")
    return out


def load_brief_pattern(path):
    with open(path) as f:
        return parse_brief_pattern(f.read())


class Latency(C.Structure):  # esvio_fe_latency
    _fields_ = [("calls", C.c_uint64), ("mean_ms", C.c_double), ("p50_ms", C.c_double), ("p99_ms", C.c_double),
                ("max_ms", C.c_double), ("max_call", C.c_uint64), ("max_published", C.c_int32),
                ("max_cpu_begin", C.c_int32), ("max_cpu_end", C.c_int32), ("max_invol_switches", C.c_int64),
                ("max_allocs", C.c_int64), ("max_phase_ms", C.c_double * LATENCY_PHASES), ("allocs", C.c_uint64),
                ("invol_switches", C.c_uint64)]


_lib = None


def lib_path():
    # (ESVIO_FE_LIB: an experimental build of the library — kernel A/B measurements under tools/_bin)
    return os.environ.get("ESVIO_FE_LIB") or os.path.join(_HERE, "libesvio_fe.so")


def load_library(build_if_missing=True):
    """dlopen libesvio_fe.so (building it in-tree if absent).  Raises if it cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if build_if_missing and not os.environ.get("ESVIO_FE_LIB") and _build.needs_build():
        _build.build()
    if not os.path.exists(path):
        raise FrontendError("libesvio_fe.so is missing: run `python -m esvio_amd.build`")
    L = C.CDLL(path)
    vp, i, d, sz = C.c_void_p, C.c_int, C.c_double, C.c_size_t
    L.esvio_fe_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.esvio_fe_destroy.argtypes = [vp]
    L.esvio_fe_reset.argtypes = [vp]
    L.esvio_fe_last_error.restype = C.c_char_p
    L.esvio_fe_last_error.argtypes = [vp]
    L.esvio_fe_version.restype = C.c_char_p
    L.esvio_fe_create_sae.argtypes = [vp, i, vp, sz, i, C.POINTER(C.c_uint64)]
    L.esvio_fe_create_sae_stereo.argtypes = [vp, vp, sz, vp, sz, i, C.POINTER(C.c_uint64)]
    L.esvio_fe_sae_to_time_surface.argtypes = [vp, i, d, vp]
    L.esvio_fe_is_corner.argtypes = [vp, vp, sz, i, vp]
    L.esvio_fe_features_to_track.argtypes = [vp, vp, sz, i, i, vp, vp, vp, C.POINTER(C.c_int32)]
    L.esvio_fe_get_sae.argtypes = [vp, i, vp, vp, vp, vp]
    L.esvio_fe_set_sae.argtypes = [vp, i, vp, vp, vp, vp]
    L.esvio_fe_calc_optical_flow_pyr_lk.argtypes = [vp, vp, vp, i, i, vp, vp, vp, i, i, i, d, i]
    L.esvio_fe_build_pyramid.argtypes = [vp, vp, i, i, i, i, vp, vp, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.esvio_fe_find_fundamental_mat.argtypes = [vp, vp, i, d, d, vp, C.POINTER(C.c_int32)]
    L.esvio_fe_lift_projective.argtypes = [C.POINTER(Camera), d, d, vp]
    L.esvio_fe_track_event.argtypes = [vp, d, vp, sz, vp, sz, i, i, C.POINTER(Tracks)]
    L.esvio_fe_track_event_mc.argtypes = [vp, d, vp, sz, vp, sz, i, i, C.POINTER(Motion),
                                          C.POINTER(Tracks)]
    L.esvio_fe_create_sae_stereo_mc.argtypes = [vp, vp, sz, vp, sz, i, C.POINTER(Motion),
                                                C.POINTER(C.c_uint64)]
    L.esvio_fe_set_next_batch.argtypes = [vp, d, vp, sz, vp, sz, i, i]
    L.esvio_fe_set_next_batch_mc.argtypes = [vp, d, vp, sz, vp, sz, i, i, C.POINTER(Motion)]
    L.esvio_fe_mem_alloc.argtypes = [i, sz, vp]
    L.esvio_fe_mem_free.argtypes = [i, vp]
    L.esvio_fe_mem_upload.argtypes = [vp, vp, sz]
    L.esvio_fe_register_host_buffer.argtypes = [vp, sz]
    L.esvio_fe_unregister_host_buffer.argtypes = [vp]
    L.esvio_fe_debug_inject.argtypes = [vp, i]
    L.esvio_fe_debug_counters.argtypes = [vp, vp]
    L.esvio_fe_plain_call_counters.argtypes = [vp, vp]
    L.esvio_fe_good_features_to_track.argtypes = [vp, vp, i, d, d, vp, vp, vp, vp]
    L.esvio_fe_track_image.argtypes = [vp, d, vp, vp, i, vp]
    L.esvio_fe_pack_track_records.argtypes = [vp, vp, vp]
    L.esvio_fe_set_lazy_new_stereo.argtypes = [vp, i]
    L.esvio_fe_set_host_threads.argtypes = [vp, i]
    L.esvio_fe_ransac_stats.argtypes = [vp, i]
    L.esvio_fe_host_hypot.argtypes = [vp, vp, i, vp]
    L.esvio_fe_host_stage_copy.argtypes = [vp, vp, C.c_size_t]
    L.esvio_fe_host_nullspace.argtypes = [vp, i, i, vp, C.POINTER(C.c_int32)]
    L.esvio_fe_find_fundamental_mat_mt.argtypes = [vp, vp, i, d, d, i, vp, C.POINTER(C.c_int32)]
    L.esvio_fe_finish.argtypes = [vp, vp]
    L.esvio_fe_get_time_surface.argtypes = [vp, i, vp]
    L.esvio_fe_export_image.argtypes = [vp, i, vp, i]
    L.esvio_fe_import_image.argtypes = [vp, i, vp, i]
    L.esvio_fe_export_level.argtypes = [vp, i, i, vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.esvio_fe_fast_corners.argtypes = [vp, i, vp, i, i, i, i, vp, vp, C.c_int32, C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32)]
    L.esvio_fe_set_detector.argtypes = [vp, i, i]
    L.esvio_fe_set_event_images.argtypes = [vp, i]
    L.esvio_fe_clear_event_images.argtypes = [vp]
    L.esvio_fe_get_event_image.argtypes = [vp, i, vp, i]
    L.esvio_fe_get_event_canvas.argtypes = [vp, vp, i]
    L.esvio_fe_event_image_kernel_stats.argtypes = [vp, i, C.POINTER(d), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.esvio_fe_features_to_track_fast.argtypes = [vp, vp, i, i, i, vp, vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.esvio_fe_select_candidates.argtypes = [vp, vp, vp, i, d, i, vp, vp, i, i, i, i, vp, vp, vp, C.POINTER(C.c_int32)]
    L.esvio_fe_convert_events.argtypes = [vp, C.POINTER(EventFieldsDesc), sz, i, vp, i, C.POINTER(C.c_uint64)]
    L.esvio_fe_track_event_fields.argtypes = [vp, d, C.POINTER(EventFieldsDesc), sz, C.POINTER(EventFieldsDesc), sz, i, i,
                                              C.POINTER(Tracks)]
    L.esvio_fe_filter_events.argtypes = [vp, i, vp, sz, i, C.c_int64, i, vp, i, C.POINTER(C.c_uint64), vp, vp,
                                         C.POINTER(C.c_uint64)]
    L.esvio_fe_filter_reset.argtypes = [vp]
    L.esvio_fe_filter_batch.argtypes = [vp, i, vp, C.POINTER(EventFieldsDesc), sz, i, C.POINTER(FilterParams), vp, i,
                                        C.POINTER(C.c_uint64), vp, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.esvio_fe_set_address_filter.argtypes = [vp, i, C.POINTER(AddressFilter)]
    L.esvio_fe_set_pixel_mask.argtypes = [vp, i, vp, sz]
    L.esvio_fe_get_pixel_mask.argtypes = [vp, i, vp, sz, C.POINTER(sz)]
    L.esvio_fe_hot_learn.argtypes = [vp, i, vp, C.POINTER(EventFieldsDesc), sz, i, C.POINTER(C.c_uint64)]
    L.esvio_fe_hot_select.argtypes = [vp, i, C.POINTER(HotParams), vp, vp, sz, C.POINTER(HotInfo)]
    L.esvio_fe_hot_reset.argtypes = [vp]
    L.esvio_fe_track_batch.argtypes = [vp, C.POINTER(Batch), C.POINTER(Tracks), C.POINTER(BatchInfo)]
    L.esvio_fe_track_event_filtered.argtypes = [vp, vp, sz, vp, sz, i, C.c_int64, i, i, C.POINTER(Tracks),
                                                C.POINTER(C.c_uint64 * 2), C.POINTER(d)]
    L.esvio_fe_decode_raw.argtypes = [vp, i, i, vp, sz, i, C.c_int64, vp, sz, i, C.POINTER(RawInfo)]
    L.esvio_fe_decode_reset.argtypes = [vp]
    L.esvio_fe_track_raw.argtypes = [vp, i, vp, sz, vp, sz, i, C.c_int64, i, C.POINTER(FilterParams), C.POINTER(Motion),
                                     C.POINTER(Tracks), C.POINTER(BatchInfo), C.POINTER(RawInfo * 2)]
    L.esvio_fe_slice_events.argtypes = [vp, i, vp, sz, i, C.POINTER(SliceParams), vp, sz, C.POINTER(SliceInfo)]
    L.esvio_fe_decode_triggers.argtypes = [vp, i, i, vp, sz, i, C.c_int64, vp, sz, C.POINTER(TriggerInfo)]
    L.esvio_fe_raw_header.argtypes = [vp, sz, C.POINTER(RawHeaderInfo)]
    L.esvio_fe_slice_events_at.argtypes = [vp, i, vp, sz, i, vp, sz, vp, sz, C.POINTER(SliceInfo)]
    L.esvio_fe_slice_flush.argtypes = [vp, i, C.POINTER(SliceInfo)]
    L.esvio_fe_slice_reset.argtypes = [vp]
    L.esvio_fe_feed_open.argtypes = [vp, C.POINTER(SliceParams), C.POINTER(FilterParams)]
    L.esvio_fe_feed_push_events.argtypes = [vp, i, vp, sz, i, C.POINTER(FeedInfo)]
    L.esvio_fe_feed_push_fields.argtypes = [vp, i, C.POINTER(EventFieldsDesc), sz, i, C.POINTER(FeedInfo)]
    L.esvio_fe_feed_push_raw.argtypes = [vp, i, i, vp, sz, i, C.c_int64, C.POINTER(FeedInfo)]
    L.esvio_fe_feed_peek.argtypes = [vp, C.POINTER(FeedWindow)]
    L.esvio_fe_decode_text.argtypes = [vp, i, C.POINTER(TextFormat), vp, sz, i, C.c_int64, vp, sz, i, C.POINTER(TextInfo)]
    L.esvio_fe_track_text.argtypes = [vp, C.POINTER(TextFormat), vp, sz, vp, sz, i, C.c_int64, i, C.POINTER(FilterParams),
                                      C.POINTER(Motion), C.POINTER(Tracks), C.POINTER(BatchInfo), C.POINTER(TextInfo * 2)]
    L.esvio_fe_feed_push_text.argtypes = [vp, i, C.POINTER(TextFormat), vp, sz, i, C.c_int64, C.POINTER(FeedInfo)]
    L.esvio_fe_text_imu.argtypes = [vp, sz, C.c_int64, vp, sz, C.POINTER(sz)]
    L.esvio_fe_text_images.argtypes = [vp, sz, C.c_int64, vp, vp, vp, sz, C.POINTER(sz)]
    L.esvio_fe_text_limits.argtypes = [C.POINTER(TextLimits)]
    L.esvio_fe_scan_lanes.argtypes = [C.POINTER(ScanLanes)]
    L.esvio_fe_text_kernel_name.argtypes = [i]
    L.esvio_fe_text_kernel_name.restype = C.c_char_p
    L.esvio_fe_text_kernel_stats.argtypes = [vp, i, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    u32 = C.c_uint32
    L.esvio_fe_aedat_header.argtypes = [vp, sz, C.POINTER(AedatHeaderInfo)]
    L.esvio_fe_decode_aedat.argtypes = [vp, i, vp, sz, C.c_int64, u32, vp, sz, i, C.POINTER(AedatInfo)]
    L.esvio_fe_aedat_side.argtypes = [vp, i, vp, sz, C.c_int64, u32, vp, sz, vp, sz, C.POINTER(AedatSideInfo)]
    L.esvio_fe_track_aedat.argtypes = [vp, vp, sz, vp, sz, C.c_int64, u32, i, C.POINTER(FilterParams), C.POINTER(Motion),
                                       C.POINTER(Tracks), C.POINTER(BatchInfo), C.POINTER(AedatInfo * 2)]
    L.esvio_fe_feed_push_aedat.argtypes = [vp, i, vp, sz, C.c_int64, u32, C.POINTER(FeedInfo)]
    L.esvio_fe_aedat_walk_tap.argtypes = [vp, sz, vp, sz, vp, sz, vp, sz, vp]
    L.esvio_fe_decode_aedat_frames.argtypes = [vp, i, vp, sz, C.c_int64, u32, vp, sz, i, vp, sz, C.POINTER(AedatFrameInfo)]
    L.esvio_fe_convert_frame16.argtypes = [vp, vp, i, u32, u32, C.c_int32, vp, i]
    L.esvio_fe_aedat_frame_walk_tap.argtypes = [vp, sz, u32, u32, vp, sz, C.c_int64, u32, vp, sz, vp, sz, vp, sz, vp, vp, sz]
    L.esvio_fe_aedat_frame_kernel_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.esvio_fe_bag_header.argtypes = [vp, sz, C.POINTER(BagHeaderInfo)]
    L.esvio_fe_bag_set_topics.argtypes = [vp, C.POINTER(BagTopics)]
    L.esvio_fe_decode_bag.argtypes = [vp, vp, sz, u32, C.POINTER(vp * 2), C.POINTER(sz * 2), i, vp, sz, C.POINTER(BagInfo)]
    L.esvio_fe_bag_side.argtypes = [vp, vp, sz, u32, vp, sz, C.POINTER(BagSideInfo)]
    L.esvio_fe_feed_push_bag.argtypes = [vp, vp, sz, u32, C.POINTER(FeedInfo * 2)]
    L.esvio_fe_bag_set_image_topics.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.esvio_fe_decode_bag_images.argtypes = [vp, vp, sz, u32, C.POINTER(vp * 2), C.POINTER(sz * 2), i, vp, sz, C.POINTER(BagImageInfo)]
    L.esvio_fe_convert_image.argtypes = [vp, vp, i, u32, u32, u32, C.c_int32, vp, i]
    L.esvio_fe_track_image_space.argtypes = [vp, d, vp, vp, i, i, vp]
    L.esvio_fe_bag_image_walk_tap.argtypes = [vp, sz, C.c_char_p, C.c_char_p, u32, u32, vp, sz, vp, sz, vp, sz, vp, sz, vp, vp, sz]
    L.esvio_fe_bag_walk_tap.argtypes = [vp, sz, C.POINTER(BagTopics), i, vp, sz, C.POINTER(vp * 2), C.POINTER(sz * 2), vp, sz, vp, sz, vp, vp, sz]
    L.esvio_fe_feed_track.argtypes = [vp, i, C.POINTER(Motion), C.POINTER(Tracks), C.POINTER(BatchInfo)]
    L.esvio_fe_feed_close.argtypes = [vp]
    L.esvio_fe_set_profiling.argtypes = [vp, i]
    L.esvio_fe_kernel_name.restype = C.c_char_p
    L.esvio_fe_kernel_name.argtypes = [i]
    L.esvio_fe_get_kernel_stats.argtypes = [vp, i, C.POINTER(d), C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64)]
    L.esvio_fe_reset_kernel_stats.argtypes = [vp]
    L.esvio_fe_stream.restype = vp
    L.esvio_fe_stream.argtypes = [vp]
    L.esvio_fe_device_memory.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
    L.esvio_fe_exchange_tracks.argtypes = [vp, vp, i, vp]
    L.esvio_fe_comm_unique_id.argtypes = [vp]
    L.esvio_fe_comm_init.argtypes = [vp, vp, i, i]
    L.esvio_fe_exchange_begin.argtypes = [vp]
    L.esvio_fe_exchange_end.argtypes = [vp, vp]
    L.esvio_fe_set_auto_exchange.argtypes = [vp, i]
    L.esvio_fe_sae_plane_doubles.restype = sz
    L.esvio_fe_sae_plane_doubles.argtypes = [vp]
    L.esvio_fe_sae_slice_last.argtypes = [vp, vp, sz, vp, sz, i, vp, i]
    L.esvio_fe_sae_slice_apply.argtypes = [vp, vp, sz, vp, sz, i, vp, i, i, vp, i]
    L.esvio_fe_sae_slice_commit.argtypes = [vp, vp, vp, i, i]
    L.esvio_fe_reserve.argtypes = [vp, sz, sz, i]
    L.esvio_fe_set_launch_thread.argtypes = [vp, i]
    L.esvio_fe_latency_stats.argtypes = [vp, C.POINTER(Latency), i]
    L.esvio_fe_latency_recent.argtypes = [vp, i, C.POINTER(LatencyCall)]
    L.esvio_fe_latency_phase_name.restype = C.c_char_p
    L.esvio_fe_latency_phase_name.argtypes = [i]
    L.esvio_fe_ransac_tail.argtypes = [vp, i]
    L.esvio_fe_find_fundamental_mat_held.argtypes = [vp, vp, i, d, d, i, i, vp, C.POINTER(C.c_int32)]
    L.esvio_fe_find_fundamental_mat_idle.argtypes = [vp, vp, i, d, d, i, i, i, vp, C.POINTER(C.c_int32), vp]
    i32p = C.POINTER(C.c_int32)
    L.esvio_fe_kf_set_pattern.argtypes = [vp, vp, vp, vp, vp, i]
    L.esvio_fe_kf_blur.argtypes = [vp, vp, i, vp, i]
    L.esvio_fe_kf_fast.argtypes = [vp, vp, i, i, vp, vp, C.c_int32, i32p, i32p]
    L.esvio_fe_kf_brief.argtypes = [vp, vp, i, vp, i, vp, i]
    L.esvio_fe_kf_match.argtypes = [vp, vp, i, vp, i, i, vp, vp, vp]
    L.esvio_fe_kf_describe.argtypes = [vp, i, vp, i, vp, i, i, C.POINTER(KfOut)]
    L.esvio_fe_kf_kernel_name.restype = C.c_char_p
    L.esvio_fe_kf_kernel_name.argtypes = [i]
    L.esvio_fe_kf_kernel_stats.argtypes = [vp, i, C.POINTER(d), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.esvio_fe_kf_blur_tile.argtypes = [i32p, i32p]
    L.esvio_fe_bow_vocabulary_header.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(BowVocabularyInfo)]
    L.esvio_fe_bow_set_vocabulary.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.esvio_fe_bow_transform.argtypes = [vp, vp, i, i, vp, vp, vp, vp, C.c_int32, i32p]
    L.esvio_fe_bow_add.argtypes = [vp, vp, i, i, i32p]
    L.esvio_fe_bow_query.argtypes = [vp, vp, i, i, i, i, C.POINTER(BowResult), i32p]
    L.esvio_fe_bow_detect_loop.argtypes = [vp, vp, i, i, i, i32p, C.POINTER(BowResult), i32p]
    L.esvio_fe_bow_clear.argtypes = [vp]
    L.esvio_fe_bow_entries.argtypes = [vp]
    L.esvio_fe_bow_reserve.argtypes = [vp, C.c_int64, C.c_int64]
    L.esvio_fe_bow_kernel_name.restype = C.c_char_p
    L.esvio_fe_bow_kernel_name.argtypes = [i]
    L.esvio_fe_bow_kernel_stats.argtypes = [vp, i, C.POINTER(d), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.esvio_fe_bow_limits.argtypes = [C.POINTER(BowLimits)]
    L.esvio_fe_bow_scores.argtypes = [vp, vp, i, i, i, vp, vp]
    L.esvio_fe_bow_create_vocabulary.argtypes = [vp, vp, C.c_int64, i, vp, C.c_int32, C.POINTER(BowCreateParams), C.POINTER(BowCreateInfo)]
    L.esvio_fe_bow_get_created.argtypes = [vp, vp, C.c_size_t]
    L.esvio_fe_bow_create_kernel_name.restype = C.c_char_p
    L.esvio_fe_bow_create_kernel_name.argtypes = [i]
    L.esvio_fe_bow_create_kernel_stats.argtypes = [vp, i, C.POINTER(d), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.esvio_fe_bow_create_pick.argtypes = [vp, vp, C.c_int64, vp, C.c_int32, vp, vp]
    L.esvio_fe_sort_pairs.argtypes = [vp, vp, vp, C.c_int64, i, i, C.c_int64, vp, vp, C.POINTER(C.c_int32), vp]
    _lib = L
    return L


# How calcOpticalFlowPyrLK's sums are accumulated when a caller does not say: 2 = in float, in the order of the
# x86 OpenCV build the reference node links (feature_tracker.cpp:410,417-418,490,495) — the reference's own
# arithmetic; 1 = exact integer sums.  ESVIO_LK_ACCUM=1 in the environment runs everything that does not say
# (the test suite, tools/) in the exact mode instead.
DEFAULT_LK_ACCUM = int(os.environ.get("ESVIO_LK_ACCUM", "2"))


def make_config(W, H, device=-1, **kw):
    """esvio_fe_config with the shipped defaults of config/esio_DSEC/esio.yaml:77-94
    (equalize forced 0) unless overridden."""
    c = Config()
    c.width, c.height = W, H
    c.decay_ms = kw.get("decay_ms", 20.0)
    c.ignore_polarity = kw.get("ignore_polarity", 0)
    c.median_blur_kernel_size = kw.get("median_blur_kernel_size", 0)
    c.feature_filter_threshold = kw.get("feature_filter_threshold", 0.01)
    c.ts_lk_threshold = kw.get("ts_lk_threshold", 128.0)
    c.max_cnt = kw.get("max_cnt", 300)
    c.min_dist = kw.get("min_dist", 10)
    c.flow_back = kw.get("flow_back", 1)
    c.equalize = kw.get("equalize", 0)
    c.f_threshold = kw.get("f_threshold", 1.0)
    c.f_ransac = kw.get("f_ransac", 1)
    c.lk_accum = kw.get("lk_accum", DEFAULT_LK_ACCUM)
    c.focal_length = kw.get("focal_length", 460)
    c.device = device
    cams = kw.get("cams")
    if cams is None:
        cams = [dict(fx=0.9 * W, fy=0.9 * W, cx=W / 2.0, cy=H / 2.0, k1=-0.05, k2=0.01, p1=1e-4,
                     p2=-2e-4)] * 2
    for k in range(2):
        for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2"):
            setattr(c.cam[k], n, float(cams[k][n]))
    return c


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


PAD = 24  # kPad (fe_kernels.h): the border kept around every pyramid level
DETECT_ARC, DETECT_FAST = 0, 1  # esvio_fe_set_detector
FAULT_TICKET, FAULT_LOOKBACK, FAULT_SPECULATIVE, FAULT_CHAINED, FAULT_LAZY_LATE = 1, 2, 4, 8, 16


def _events_arg(ev):
    """numpy EVENT_DTYPE array -> (pointer, n, HOST); (device_ptr:int, n) tuple -> DEVICE."""
    if isinstance(ev, tuple):
        return C.c_void_p(ev[0]), int(ev[1]), DEVICE, None
    ev = np.ascontiguousarray(ev)
    if ev.dtype.itemsize != 16:
        raise ValueError("events must be 16-byte records (esvio_amd.events.EVENT_DTYPE)")
    return _p(ev), ev.shape[0], HOST, ev


class _Handle:
    def __init__(self, cfg):
        self.L = load_library()
        self.cfg = cfg
        h = C.c_void_p()
        rc = self.L.esvio_fe_create(C.byref(cfg), C.byref(h))
        if rc != 0 or not h:
            raise FrontendError("esvio_fe_create failed rc=%d (no GPU / bad config)" % rc)
        self.h = h

    def check(self, rc):
        if rc != 0:
            raise FrontendError("rc=%d: %s" % (rc, self.L.esvio_fe_last_error(self.h).decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.esvio_fe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EventDetector:
    """esvio::EventDetector (event_detector.h:18-80) — batch forms of its per-event methods."""

    def __init__(self, cfg=None, handle=None, **kw):
        if handle is None:
            handle = _Handle(cfg if cfg is not None else make_config(**kw))
        self._hd = handle
        self.W, self.H = handle.cfg.width, handle.cfg.height

    def createSAE_left(self, events):
        return self._create_sae(0, events)

    def createSAE_right(self, events):
        return self._create_sae(1, events)

    def _create_sae(self, cam, events):
        ptr, n, space, keep = _events_arg(events)
        rej = C.c_uint64(0)
        self._hd.check(self._hd.L.esvio_fe_create_sae(self._hd.h, cam, ptr, n, space, C.byref(rej)))
        return rej.value

    def createSAE_stereo(self, left, right):
        pl, nl, sl, k1 = _events_arg(left)
        pr, nr, sr, k2 = _events_arg(right)
        assert sl == sr
        rej = C.c_uint64(0)
        self._hd.check(self._hd.L.esvio_fe_create_sae_stereo(self._hd.h, pl, nl, pr, nr, sl,
                                                             C.byref(rej)))
        return rej.value

    def createSAE_stereo_mc(self, left, right, motion):
        """createSAE_left/right(et, ex, ey, ep, measurements) loops (feature_tracker.cpp:627-641)"""
        pl, nl, sl, k1 = _events_arg(left)
        pr, nr, sr, k2 = _events_arg(right)
        assert sl == sr
        rej = C.c_uint64(0)
        self._hd.check(self._hd.L.esvio_fe_create_sae_stereo_mc(self._hd.h, pl, nl, pr, nr, sl,
                                                                C.byref(motion), C.byref(rej)))
        return rej.value

    def SAEtoTimeSurface_left(self, external_sync_time):
        return self._ts(0, external_sync_time)

    def SAEtoTimeSurface_right(self, external_sync_time):
        return self._ts(1, external_sync_time)

    def _ts(self, cam, t):
        out = np.empty((self.H, self.W), np.uint8)
        self._hd.check(self._hd.L.esvio_fe_sae_to_time_surface(self._hd.h, cam, float(t), _p(out)))
        return out

    def isCorner(self, events):
        """isCorner(e.ts.toSec(), e.x, e.y, e.polarity) for every event -> uint8 flags."""
        ptr, n, space, keep = _events_arg(events)
        flags = np.zeros(n, np.uint8)
        self._hd.check(self._hd.L.esvio_fe_is_corner(self._hd.h, ptr, n, space, _p(flags)))
        return flags

    def event_image(self, cam):
        """detector.cur_event_mat_left / _right (event_detector.cc:145-146, :208-209) as (H, W, 3) uint8, B G R
        (esvio_fe_get_event_image; esvio_fe_set_event_images must be on)"""
        out = np.empty((self.H, self.W, 3), np.uint8)
        self._hd.check(self._hd.L.esvio_fe_get_event_image(self._hd.h, int(cam), _p(out), HOST))
        return out

    @property
    def cur_event_mat_left(self):
        return self.event_image(0)

    @property
    def cur_event_mat_right(self):
        return self.event_image(1)

    def get_sae(self, cam):
        planes = [np.empty((self.H, self.W), np.float64) for _ in range(4)]
        self._hd.check(self._hd.L.esvio_fe_get_sae(self._hd.h, cam, *[_p(a) for a in planes]))
        return planes  # L0, L1, S0, S1

    def set_sae(self, cam, L0, L1, S0, S1):
        arrs = [np.ascontiguousarray(a, np.float64) for a in (L0, L1, S0, S1)]
        self._hd.check(self._hd.L.esvio_fe_set_sae(self._hd.h, cam, *[_p(a) for a in arrs]))


class FeatureTracker:
    """FeatureTracker (feature_tracker.h:49-173): trackEvent + the public result members."""

    def __init__(self, cfg=None, **kw):
        self.cfg = cfg if cfg is not None else make_config(**kw)
        self._hd = _Handle(self.cfg)
        self.detector = EventDetector(handle=self._hd)
        m = max(self.cfg.max_cnt, 1)
        self._bufs = dict(
            ids=np.zeros(m, np.int32), track_cnt=np.zeros(m, np.int32),
            cur_pts=np.zeros((m, 2), np.float32), cur_un_pts=np.zeros((m, 2), np.float32),
            pts_velocity=np.zeros((m, 2), np.float32),
            ids_right=np.zeros(m, np.int32), cur_right_pts=np.zeros((m, 2), np.float32),
            cur_un_right_pts=np.zeros((m, 2), np.float32),
            right_pts_velocity=np.zeros((m, 2), np.float32))
        self._tr = Tracks()
        for k, a in self._bufs.items():
            setattr(self._tr, k, a.ctypes.data)
        self._copy = False

    def close(self):
        self._hd.close()

    def trackEvent(self, cur_time, event_left, event_right, PUB_THIS_FRAME=True, copy=True,
                   measurements=None):
        """both overloads of FeatureTracker::trackEvent (feature_tracker.h:51-52); `measurements`
        is an esvio_fe_motion (frontend.make_motion) for the motion-compensated one"""
        pl, nl, sl, k1 = _events_arg(event_left)
        pr, nr, sr, k2 = _events_arg(event_right)
        assert sl == sr
        if measurements is None:
            self._hd.check(self._hd.L.esvio_fe_track_event(
                self._hd.h, float(cur_time), pl, nl, pr, nr, sl, int(PUB_THIS_FRAME), C.byref(self._tr)))
        else:
            self._hd.check(self._hd.L.esvio_fe_track_event_mc(
                self._hd.h, float(cur_time), pl, nl, pr, nr, sl, int(PUB_THIS_FRAME),
                C.byref(measurements), C.byref(self._tr)))
        return self._take(copy)

    def set_event_images(self, on):
        """show_track's event images (esvio_fe_set_event_images): every track and stage call from now on keeps
        detector.cur_event_mat_left/right on the device; allocates (on) or releases (off) their memory.  on = 2
        (EVENT_IMAGES_AHEAD): the images follow announced batches (set_next_batch is accepted), at 62 bytes per pixel"""
        self._hd.check(self._hd.L.esvio_fe_set_event_images(self._hd.h, EVENT_IMAGES_AHEAD if on == EVENT_IMAGES_AHEAD else int(bool(on))))

    def clear_event_images(self):
        """the Mat::zeros of feature_tracker.cpp:352-353 (esvio_fe_clear_event_images)"""
        self._hd.check(self._hd.L.esvio_fe_clear_event_images(self._hd.h))

    def event_image(self, cam):
        """(H, W, 3) uint8, B G R: the camera's event image after the latest call"""
        return self.detector.event_image(cam)

    def event_canvas(self):
        """hconcat(cur_event_mat_left, cur_event_mat_right) (feature_tracker.cpp:1107), the base of feature_img, as
        (H, 2 W, 3) uint8 (esvio_fe_get_event_canvas)"""
        out = np.empty((self.cfg.height, 2 * self.cfg.width, 3), np.uint8)
        self._hd.check(self._hd.L.esvio_fe_get_event_canvas(self._hd.h, _p(out), HOST))
        return out

    def convert_events(self, fields, space=DEVICE, src_space=HOST):
        """events.EventFields -> event records, converted on the device (esvio_fe_convert_events).  Returns a
        ConvertedEvents with EventBuffer's contract: `.arg` (space DEVICE: what every entry point takes for device
        events, set_next_batch included) or `.array` (space HOST: a numpy EVENT_DTYPE array), and `.free()`.
        src_space DEVICE: the fields' pointers are device addresses (EventFields.at_pointers).  A stamp that falls
        outside [0, 2^32 s) raises FrontendError; `.n_bad` of the exception holds the count."""
        return ConvertedEvents(self._hd, fields, space, src_space)

    def trackEventFields(self, cur_time, left_fields, right_fields, PUB_THIS_FRAME=True, copy=True, src_space=HOST):
        """trackEvent for events.EventFields of the two cameras (esvio_fe_track_event_fields): converted into
        buffers of the handle, then tracked as device events"""
        dl, dr = fields_desc(left_fields), fields_desc(right_fields)
        self._hd.check(self._hd.L.esvio_fe_track_event_fields(
            self._hd.h, float(cur_time), C.byref(dl), left_fields.n, C.byref(dr), right_fields.n, src_space,
            int(PUB_THIS_FRAME), C.byref(self._tr)))
        return self._take(copy)

    def filter_events(self, cam, ev, window_ns, min_support=1, device=False):
        """the background-activity filter stage (esvio_fe_filter_events; include/esvio_fe.h has the rule): advances
        camera `cam`'s stamp plane by the events `ev` (a numpy EVENT_DTYPE array, or a (device_ptr, n) tuple) and
        returns (kept, flags, n_rejected).  kept: the kept records in stream order — a numpy array, or with
        device=True a FilteredEvents in device memory (`.arg`: what every entry point takes for device events,
        set_next_batch included; `.n`, `.last`: the last kept record or None; `.free()`).  flags: keep_i per event."""
        from .events import EVENT_DTYPE
        ptr, n, space, keep = _events_arg(ev)
        flags = np.zeros(n, np.uint8)
        nk, rej = C.c_uint64(0), C.c_uint64(0)
        last = np.zeros(1, EVENT_DTYPE)
        L = self._hd.L
        if device:
            dst = C.c_void_p()
            rc = L.esvio_fe_mem_alloc(DEVICE, 16 * max(n, 1), C.byref(dst))
            if rc:
                raise FrontendError("esvio_fe_mem_alloc rc=%d" % rc)
            out = None
        else:
            out = np.zeros(n, EVENT_DTYPE)
            dst = _p(out)
        rc = L.esvio_fe_filter_events(self._hd.h, int(cam), ptr, n, space, int(window_ns), int(min_support), dst,
                                      DEVICE if device else HOST, C.byref(nk), _p(flags), _p(last), C.byref(rej))
        if rc and device:
            L.esvio_fe_mem_free(DEVICE, dst)
        self._hd.check(rc)
        k = int(nk.value)
        kept = FilteredEvents(dst, k, last[0] if k else None) if device else out[:k]
        return kept, flags, int(rej.value)

    def filter_batch(self, cam, ev, params, device=False, src_space=HOST):
        """the filter stage with FilterParams (esvio_fe_filter_batch): `ev` is a numpy EVENT_DTYPE array, a
        (device_ptr, n) tuple or an events.EventFields (read where they lie: `src_space` says where; no record of an
        event that is not kept is made).  Returns (kept, flags, n_rejected) as filter_events does.  A BAD event in the
        fields raises FrontendError with `.n_bad`; the camera's plane is then as it was."""
        from .events import EVENT_DTYPE, EventFields
        L = self._hd.L
        if isinstance(ev, EventFields):
            desc = fields_desc(ev)
            ptr, fptr, n, space = None, C.byref(desc), ev.n, src_space
        else:
            ptr, n, space, keep = _events_arg(ev)
            fptr = None
        flags = np.zeros(n, np.uint8)
        nk, rej, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        last = np.zeros(1, EVENT_DTYPE)
        if device:
            dst = C.c_void_p()
            rc = L.esvio_fe_mem_alloc(DEVICE, 16 * max(n, 1), C.byref(dst))
            if rc:
                raise FrontendError("esvio_fe_mem_alloc rc=%d" % rc)
            out = None
        else:
            out = np.zeros(n, EVENT_DTYPE)
            dst = _p(out)
        rc = L.esvio_fe_filter_batch(self._hd.h, int(cam), ptr, fptr, n, space, C.byref(params), dst,
                                     DEVICE if device else HOST, C.byref(nk), _p(flags), _p(last), C.byref(rej), C.byref(bad))
        if rc and device:
            L.esvio_fe_mem_free(DEVICE, dst)
        if rc:
            e = FrontendError("rc=%d: %s" % (rc, L.esvio_fe_last_error(self._hd.h).decode()))
            e.n_bad = int(bad.value)
            raise e
        k = int(nk.value)
        kept = FilteredEvents(dst, k, last[0] if k else None) if device else out[:k]
        return kept, flags, int(rej.value)

    def set_address_filter(self, cam, address_filter):
        """camera `cam`'s address stage (esvio_fe_set_address_filter): an AddressFilter, or None for none.  A setting:
        it survives reset() and filter_reset() and runs wherever FilterParams run"""
        self._hd.check(self._hd.L.esvio_fe_set_address_filter(
            self._hd.h, int(cam), C.byref(address_filter) if address_filter is not None else None))

    def set_pixel_mask(self, cam, xy):
        """camera `cam`'s pixel mask: `xy` an (n, 2) array of (x, y) pairs; empty clears it"""
        a = np.ascontiguousarray(np.asarray(xy, np.uint16).reshape(-1, 2))
        self._hd.check(self._hd.L.esvio_fe_set_pixel_mask(self._hd.h, int(cam), _p(a) if len(a) else None, len(a)))

    def pixel_mask(self, cam):
        """camera `cam`'s masked pixels as an (n, 2) uint16 array of (x, y), in raster order"""
        L, n = self._hd.L, C.c_size_t(0)
        L.esvio_fe_get_pixel_mask(self._hd.h, int(cam), None, 0, C.byref(n))  # (the count; EINVAL when it is not 0)
        out = np.zeros((n.value, 2), np.uint16)
        if n.value:
            self._hd.check(L.esvio_fe_get_pixel_mask(self._hd.h, int(cam), _p(out), n.value, C.byref(n)))
        return out[:n.value]

    def hot_learn(self, cam, ev, src_space=HOST):
        """counts camera `cam`'s events per pixel (esvio_fe_hot_learn): `ev` as filter_batch takes it.  A BAD event in
        the fields raises FrontendError with `.n_bad`; the other events of the call are counted"""
        from .events import EventFields
        L, bad = self._hd.L, C.c_uint64(0)
        if isinstance(ev, EventFields):
            desc = fields_desc(ev)
            rc = L.esvio_fe_hot_learn(self._hd.h, int(cam), None, C.byref(desc), ev.n, src_space, C.byref(bad))
        else:
            ptr, n, space, keep = _events_arg(ev)
            rc = L.esvio_fe_hot_learn(self._hd.h, int(cam), ptr, None, n, space, C.byref(bad))
        if rc:
            e = FrontendError("rc=%d: %s" % (rc, L.esvio_fe_last_error(self._hd.h).decode()))
            e.n_bad = int(bad.value)
            raise e

    def hot_select(self, cam, params, cap=None):
        """the hottest pixels of what camera `cam` has learned (esvio_fe_hot_select; params: a HotParams) ->
        (xy (n, 2) uint16, counts uint32[n], HotInfo): count descending, then pixel index ascending"""
        cap = int(params.max_pixels if cap is None else cap)
        xy, counts, info = np.zeros((max(cap, 1), 2), np.uint16), np.zeros(max(cap, 1), np.uint32), HotInfo()
        rc = self._hd.L.esvio_fe_hot_select(self._hd.h, int(cam), C.byref(params), _p(xy), _p(counts), cap, C.byref(info))
        if rc:
            e = FrontendError("rc=%d: %s" % (rc, self._hd.L.esvio_fe_last_error(self._hd.h).decode()))
            e.info = info
            raise e
        return xy[:info.selected].copy(), counts[:info.selected].copy(), info

    def hot_reset(self):
        """hot-pixel learning: nothing counted, both cameras"""
        self._hd.check(self._hd.L.esvio_fe_hot_reset(self._hd.h))

    def track_batch(self, left, right, cur_time=None, pub=True, params=None, measurements=None, copy=True, src_space=HOST):
        """one batch through esvio_fe_track_batch: left / right are numpy EVENT_DTYPE arrays, (device_ptr, n) tuples or
        events.EventFields (per camera one kind; `src_space` says where fields lie); params: a FilterParams or None;
        measurements: an esvio_fe_motion or None; cur_time None: the stamp of the last left record the tracker is
        given.  Returns the BatchInfo: .kept, .rejected, .bad, .cur_time, .tracked (0: no left record was kept, the
        result members are the previous call's)."""
        from .events import EventFields
        b, keep, spaces = Batch(), [], []
        for side, ev in (("left", left), ("right", right)):
            if isinstance(ev, EventFields):
                d = fields_desc(ev)
                keep.append(d)
                setattr(b, side + "_fields", C.pointer(d))
                n = ev.n
                spaces.append(src_space)
            else:
                ptr, n, sp, k = _events_arg(ev)
                keep.append(k)
                setattr(b, side, ptr)
                if n:
                    spaces.append(sp)
            setattr(b, "nL" if side == "left" else "nR", n)
        assert len(set(spaces)) <= 1, "both cameras' batches lie in one memory space"
        b.space = spaces[0] if spaces else HOST
        b.pub_this_frame = int(pub)
        if params is not None:
            b.filter = C.pointer(params)
        if measurements is not None:
            b.motion = C.pointer(measurements)
        b.cur_time_from_batch = int(cur_time is None)
        b.cur_time = 0.0 if cur_time is None else float(cur_time)
        info = BatchInfo()
        rc = self._hd.L.esvio_fe_track_batch(self._hd.h, C.byref(b), C.byref(self._tr), C.byref(info))
        if rc:
            e = FrontendError("rc=%d: %s" % (rc, self._hd.L.esvio_fe_last_error(self._hd.h).decode()))
            e.info = info
            raise e
        if info.tracked:
            self._take(copy)
        return info

    def decode_raw(self, cam, fmt, words, t_offset_us=0, dst_cap=None, device=False):
        """the raw-stream decode stage (esvio_fe_decode_raw; include/esvio_fe.h has the rule): camera `cam`'s decoder
        state advanced by `words` — a contiguous numpy array of raw words (any dtype: its bytes are the stream) or a
        (device_ptr, n_bytes) tuple — of format RAW_EVT2 / RAW_EVT3 / RAW_EVT21.  Returns (records, RawInfo): records a numpy
        EVENT_DTYPE array, or with device=True a FilteredEvents in device memory (`.arg`, `.n`, `.free()`).  dst_cap
        None: room for every record the words can stand for.  A failed call raises FrontendError with `.info`."""
        from .events import EVENT_DTYPE
        L = self._hd.L
        if isinstance(words, tuple):
            ptr, nbytes, space = C.c_void_p(words[0]), int(words[1]), DEVICE
        else:
            words = np.ascontiguousarray(words)
            ptr, nbytes, space = _p(words), words.nbytes, HOST
        if dst_cap is None:
            dst_cap = raw_bound(fmt, nbytes)
        info = RawInfo()
        if device:
            dst = C.c_void_p()
            rc = L.esvio_fe_mem_alloc(DEVICE, 16 * max(dst_cap, 1), C.byref(dst))
            if rc:
                raise FrontendError("esvio_fe_mem_alloc rc=%d" % rc)
            out = None
        else:
            out = np.zeros(dst_cap, EVENT_DTYPE)
            dst = _p(out)
        rc = L.esvio_fe_decode_raw(self._hd.h, int(cam), int(fmt), ptr, nbytes, space, int(t_offset_us), dst, int(dst_cap),
                                   DEVICE if device else HOST, C.byref(info))
        if rc:
            if device:
                L.esvio_fe_mem_free(DEVICE, dst)
            e = FrontendError("rc=%d: %s" % (rc, L.esvio_fe_last_error(self._hd.h).decode()))
            e.info = info
            raise e
        k = int(info.events)
        return (FilteredEvents(dst, k, None) if device else out[:k]), info

    def decode_text(self, cam, order, time, data, flags=0, t_offset_ns=0, dst_cap=None, device=False):
        """the text decode stage (esvio_fe_decode_text; include/esvio_fe.h "text event files" has the rule): camera
        `cam`'s text state advanced by `data` — bytes, a contiguous numpy array or a (device_ptr, n_bytes) tuple; the
        chunk may end anywhere — of a file with columns `order` (TEXT_TXYP / TEXT_XYPT) and stamps `time`
        (TEXT_SEC_DECIMAL / TEXT_INT_US / TEXT_INT_NS); flags: TEXT_END | TEXT_SKIP_MALFORMED.  Returns (records,
        TextInfo) as decode_raw does.  dst_cap None: text_bound(n_bytes).  A failed call raises FrontendError with `.info`."""
        from .events import EVENT_DTYPE
        L = self._hd.L
        ptr, nbytes, space, keep = _text_src(data)
        if dst_cap is None:
            dst_cap = text_bound(nbytes)
        fmt, info = TextFormat(int(order), int(time), int(flags), 0), TextInfo()
        if device:
            dst = C.c_void_p()
            rc = L.esvio_fe_mem_alloc(DEVICE, 16 * max(dst_cap, 1), C.byref(dst))
            if rc:
                raise FrontendError("esvio_fe_mem_alloc rc=%d" % rc)
            out = None
        else:
            out = np.zeros(max(int(dst_cap), 1), EVENT_DTYPE)
            dst = _p(out)
        rc = L.esvio_fe_decode_text(self._hd.h, int(cam), C.byref(fmt), ptr, nbytes, space, int(t_offset_ns), dst, int(dst_cap),
                                    DEVICE if device else HOST, C.byref(info))
        if rc:
            if device:
                L.esvio_fe_mem_free(DEVICE, dst)
            e = FrontendError("rc=%d: %s" % (rc, L.esvio_fe_last_error(self._hd.h).decode()))
            e.info = info
            raise e
        k = int(info.events)
        return (FilteredEvents(dst, k, None) if device else out[:k]), info

    def track_text(self, order, time, left, right, flags=0, t_offset_ns=0, pub=True, params=None, measurements=None, copy=True):
        """one chunk of text per camera through esvio_fe_track_text: left / right as decode_text takes them (both in
        one memory space); params: a FilterParams or None; measurements: an esvio_fe_motion or None.  Returns
        (BatchInfo, (TextInfo, TextInfo)); a failed call raises FrontendError with `.info` and `.text`."""
        args, spaces, keep = [], [], []
        for w in (left, right):
            ptr, nbytes, space, k = _text_src(w)
            keep.append(k)
            args += [ptr, nbytes]
            if nbytes:
                spaces.append(space)
        assert len(set(spaces)) <= 1, "both cameras' chunks lie in one memory space"
        fmt, info, text = TextFormat(int(order), int(time), int(flags), 0), BatchInfo(), (TextInfo * 2)()
        rc = self._hd.L.esvio_fe_track_text(self._hd.h, C.byref(fmt), *args, spaces[0] if spaces else HOST, int(t_offset_ns), int(pub),
                                            C.byref(params) if params is not None else None,
                                            C.byref(measurements) if measurements is not None else None,
                                            C.byref(self._tr), C.byref(info), C.byref(text))
        if rc:
            e = FrontendError("rc=%d: %s" % (rc, self._hd.L.esvio_fe_last_error(self._hd.h).decode()))
            e.info, e.text = info, text
            raise e
        if info.tracked:
            self._take(copy)
        return info, (text[0], text[1])

    def decode_reset(self):
        """both cameras' raw-stream decoder states — the event decoder's and the trigger decoder's — back to the fresh
        state (esvio_fe_decode_reset)"""
        self._hd.check(self._hd.L.esvio_fe_decode_reset(self._hd.h))

    def decode_triggers(self, cam, fmt, words, t_offset_us=0, dst_cap=None):
        """the EXT_TRIGGER words of a chunk as trigger records (esvio_fe_decode_triggers; include/esvio_fe.h has the
        rule): camera `cam`'s trigger-decoder state advanced by `words`, given as decode_raw takes them.  Returns
        (triggers, TriggerInfo): triggers a numpy TRIGGER_DTYPE array.  dst_cap None: one record per word.  A failed call
        raises FrontendError with `.info`."""
        L = self._hd.L
        if isinstance(words, tuple):
            ptr, nbytes, space = C.c_void_p(words[0]), int(words[1]), DEVICE
        else:
            words = np.ascontiguousarray(words)
            ptr, nbytes, space = _p(words), words.nbytes, HOST
        if dst_cap is None:
            dst_cap = nbytes // RAW_WORD_BYTES.get(fmt, 2)
        info = TriggerInfo()
        out = np.zeros(max(int(dst_cap), 1), TRIGGER_DTYPE)
        rc = L.esvio_fe_decode_triggers(self._hd.h, int(cam), int(fmt), ptr, nbytes, space, int(t_offset_us), _p(out), int(dst_cap),
                                        C.byref(info))
        if rc:
            e = FrontendError("rc=%d: %s" % (rc, L.esvio_fe_last_error(self._hd.h).decode()))
            e.info = info
            raise e
        return out[:int(info.triggers)], info

    def track_raw(self, fmt, left, right, t_offset_us=0, pub=True, params=None, measurements=None, copy=True):
        """one batch of raw words per camera through esvio_fe_track_raw: left / right are contiguous numpy arrays of raw
        words or (device_ptr, n_bytes) tuples (both in one memory space); params: a FilterParams or None; measurements:
        an esvio_fe_motion or None.  Returns (BatchInfo, (RawInfo, RawInfo)); a failed call raises FrontendError with
        `.info` and `.raw`."""
        args, spaces, keep = [], [], []
        for w in (left, right):
            if isinstance(w, tuple):
                args += [C.c_void_p(w[0]), int(w[1])]
                spaces.append(DEVICE)
            else:
                w = np.ascontiguousarray(w)
                keep.append(w)
                args += [_p(w), w.nbytes]
                if w.nbytes:
                    spaces.append(HOST)
        assert len(set(spaces)) <= 1, "both cameras' words lie in one memory space"
        info, raw = BatchInfo(), (RawInfo * 2)()
        rc = self._hd.L.esvio_fe_track_raw(self._hd.h, int(fmt), *args, spaces[0] if spaces else HOST, int(t_offset_us), int(pub),
                                           C.byref(params) if params is not None else None,
                                           C.byref(measurements) if measurements is not None else None,
                                           C.byref(self._tr), C.byref(info), C.byref(raw))
        if rc:
            e = FrontendError("rc=%d: %s" % (rc, self._hd.L.esvio_fe_last_error(self._hd.h).decode()))
            e.info, e.raw = info, raw
            raise e
        if info.tracked:
            self._take(copy)
        return info, (raw[0], raw[1])

    def decode_aedat(self, cam, data, t_offset_ns=0, flags=0, dst_cap=None, device=False):
        """the AEDAT 3.1 decode stage (esvio_fe_decode_aedat; include/esvio_fe.h has the rule): camera `cam`'s event
        walker advanced by `data` — bytes or a contiguous numpy array, host memory; the chunk may end anywhere.  Returns
        (records, AedatInfo) as decode_raw does.  dst_cap None: one record per 8 bytes of the chunk, and one for a record
        the last chunk cut.  A failed call raises FrontendError with `.info`."""
        from .events import EVENT_DTYPE
        L = self._hd.L
        buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data)
        if dst_cap is None:
            dst_cap = buf.nbytes // 8 + 1
        info = AedatInfo()
        if device:
            dst = C.c_void_p()
            rc = L.esvio_fe_mem_alloc(DEVICE, 16 * max(dst_cap, 1), C.byref(dst))
            if rc:
                raise FrontendError("esvio_fe_mem_alloc rc=%d" % rc)
            out = None
        else:
            out = np.zeros(max(int(dst_cap), 1), EVENT_DTYPE)
            dst = _p(out)
        rc = L.esvio_fe_decode_aedat(self._hd.h, int(cam), _p(buf) if buf.nbytes else None, buf.nbytes, int(t_offset_ns), int(flags),
                                     dst, int(dst_cap), DEVICE if device else HOST, C.byref(info))
        if rc:
            if device:
                L.esvio_fe_mem_free(DEVICE, dst)
            e = FrontendError("rc=%d: %s" % (rc, L.esvio_fe_last_error(self._hd.h).decode()))
            e.info = info
            raise e
        k = int(info.events)
        return (FilteredEvents(dst, k, None) if device else out[:k]), info

    def aedat_side(self, cam, data, t_offset_ns=0, flags=0, imu_cap=None, trig_cap=None):
        """the IMU6 samples and external-input specials of an AEDAT 3.1 chunk (esvio_fe_aedat_side): camera `cam`'s side
        walker advanced by `data`.  Returns (imu, triggers, AedatSideInfo): numpy IMU_DTYPE and TRIGGER_DTYPE arrays.
        Capacities None: what the chunk can hold at the most.  A failed call raises FrontendError with `.info`."""
        L = self._hd.L
        buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data)
        imu_cap = buf.nbytes // 36 + 1 if imu_cap is None else int(imu_cap)
        trig_cap = buf.nbytes // 8 + 1 if trig_cap is None else int(trig_cap)
        imu, trig, info = np.zeros(max(imu_cap, 1), IMU_DTYPE), np.zeros(max(trig_cap, 1), TRIGGER_DTYPE), AedatSideInfo()
        rc = L.esvio_fe_aedat_side(self._hd.h, int(cam), _p(buf) if buf.nbytes else None, buf.nbytes, int(t_offset_ns), int(flags),
                                   _p(imu), imu_cap, _p(trig), trig_cap, C.byref(info))
        if rc:
            e = FrontendError("rc=%d: %s" % (rc, L.esvio_fe_last_error(self._hd.h).decode()))
            e.info = info
            raise e
        return imu[:int(info.imu)], trig[:int(info.triggers)], info

    def decode_aedat_frames(self, cam, data, t_offset_ns=0, flags=0, dst_cap=None, frames_cap=None, device=False):
        """the AEDAT 3.1 frame call (esvio_fe_decode_aedat_frames; include/esvio_fe.h "AEDAT 3.1 frames" has the rule):
        camera `cam`'s frame walker advanced by `data`, host memory, which may end anywhere.  Returns (images, table,
        AedatFrameInfo): a numpy uint8 array [n, height, width] of gray images, or with device=True a DeviceImages (the
        caller frees it; `.image(k)` is the pointer trackImage(..., device=True) takes); table a numpy AEDAT_FRAME_DTYPE
        array whose `index` is the frame's image.  dst_cap, frames_cap None: what the chunk and the bytes that wait can
        complete at the most.  A failed call raises FrontendError with `.info`."""
        L = self._hd.L
        W, H = self.cfg.width, self.cfg.height
        buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data)
        most = buf.nbytes // (2 * W * H) + 1  # (an emitted frame brings 2 * width * height pixel bytes at the least; one may have waited)
        dst_cap = most if dst_cap is None else int(dst_cap)
        frames_cap = most if frames_cap is None else int(frames_cap)
        table, info = np.zeros(max(frames_cap, 1), AEDAT_FRAME_DTYPE), AedatFrameInfo()
        if device:
            d = C.c_void_p()
            rc = L.esvio_fe_mem_alloc(DEVICE, W * H * max(dst_cap, 1), C.byref(d))
            if rc:
                raise FrontendError("esvio_fe_mem_alloc rc=%d" % rc)
            out, dp = d, d
        else:
            out = np.zeros((max(dst_cap, 1), H, W), np.uint8)
            dp = _p(out)
        rc = L.esvio_fe_decode_aedat_frames(self._hd.h, int(cam), _p(buf) if buf.nbytes else None, buf.nbytes, int(t_offset_ns), int(flags),
                                            dp, dst_cap, DEVICE if device else HOST, _p(table), frames_cap, C.byref(info))
        if rc:
            if device:
                L.esvio_fe_mem_free(DEVICE, out)
            e = FrontendError("rc=%d: %s" % (rc, L.esvio_fe_last_error(self._hd.h).decode()))
            e.info = info
            raise e
        n = int(info.frames)
        return (DeviceImages(out, n, W, H) if device else out[:n]), table[:n], info

    def convert_frame16(self, src, height, width, channels, src_space=HOST, device=False):
        """the driver's per-frame conversion alone (esvio_fe_convert_frame16): `src` a numpy uint16 array (host) or a
        device pointer (src_space=DEVICE, 2-byte aligned) of height x width pixels of `channels` (1 or 3) values each.
        Returns the gray image [height, width], or with device=True a DeviceImages of one image (the caller frees it)."""
        L = self._hd.L
        if isinstance(src, np.ndarray):
            src = np.ascontiguousarray(src, "<u2")
        sp = _p(src) if isinstance(src, np.ndarray) else C.c_void_p(int(src))
        if device:
            d = C.c_void_p()
            rc = L.esvio_fe_mem_alloc(DEVICE, max(int(height) * int(width), 1), C.byref(d))
            if rc:
                raise FrontendError("esvio_fe_mem_alloc rc=%d" % rc)
            out, dp = DeviceImages(d, 1, int(width), int(height)), d
        else:
            out = np.zeros((int(height), int(width)), np.uint8)
            dp = _p(out)
        rc = L.esvio_fe_convert_frame16(self._hd.h, sp, int(src_space), int(height), int(width), int(channels), dp, DEVICE if device else HOST)
        if rc:
            if device:
                out.free()
            raise FrontendError("rc=%d: %s" % (rc, L.esvio_fe_last_error(self._hd.h).decode()))
        return out

    def track_aedat(self, left, right, t_offset_ns=0, flags=0, pub=True, params=None, measurements=None, copy=True):
        """one chunk of AEDAT 3.1 bytes per camera through esvio_fe_track_aedat (host memory).  Returns
        (BatchInfo, (AedatInfo, AedatInfo)); a failed call raises FrontendError with `.info` and `.aedat`."""
        args, keep = [], []
        for w in (left, right):
            w = np.frombuffer(w, np.uint8) if isinstance(w, (bytes, bytearray, memoryview)) else np.ascontiguousarray(w)
            keep.append(w)
            args += [_p(w) if w.nbytes else None, w.nbytes]
        info, ae = BatchInfo(), (AedatInfo * 2)()
        rc = self._hd.L.esvio_fe_track_aedat(self._hd.h, *args, int(t_offset_ns), int(flags), int(pub),
                                             C.byref(params) if params is not None else None,
                                             C.byref(measurements) if measurements is not None else None,
                                             C.byref(self._tr), C.byref(info), C.byref(ae))
        if rc:
            e = FrontendError("rc=%d: %s" % (rc, self._hd.L.esvio_fe_last_error(self._hd.h).decode()))
            e.info, e.aedat = info, ae
            raise e
        if info.tracked:
            self._take(copy)
        return info, (ae[0], ae[1])

    def feed_push_aedat(self, cam, data, t_offset_ns=0, flags=0):
        """append the polarity events of a chunk of AEDAT 3.1 bytes (host memory; the chunk may end anywhere)"""
        buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data)
        info = FeedInfo()
        return self._feed_pushed(self._hd.L.esvio_fe_feed_push_aedat(self._hd.h, int(cam), _p(buf) if buf.nbytes else None, buf.nbytes,
                                                                     int(t_offset_ns), int(flags), C.byref(info)), info)

    def bag_set_topics(self, left=None, right=None, imu=None):
        """which topics of a rosbag hold the left and right dvs_msgs/EventArray messages and the sensor_msgs/Imu messages
        (esvio_fe_bag_set_topics; None: none).  Clears both bag walker states."""
        self._hd.check(self._hd.L.esvio_fe_bag_set_topics(self._hd.h, C.byref(_bag_topics(left, right, imu))))

    def decode_bag(self, data, dst_cap=None, msgs_cap=None, device=False, flags=0):
        """the rosbag decode stage (esvio_fe_decode_bag; include/esvio_fe.h has the rule): the event walker advanced by
        `data` — bytes or a contiguous numpy array, host memory, from the bag's payload_offset on; the chunk may end
        anywhere.  Returns ((left, right), messages, BagInfo): per camera a numpy EVENT_DTYPE array, or with device=True a
        FilteredEvents (the caller frees it); messages a numpy BAG_MESSAGE_DTYPE array.  dst_cap None: one record per 13
        bytes of the chunk, and one for an event the last chunk cut; a number or a pair.  A failed call raises
        FrontendError with `.info`."""
        from .events import EVENT_DTYPE
        L = self._hd.L
        buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data)
        if dst_cap is None:
            dst_cap = buf.nbytes // 13 + 1
        caps = [int(dst_cap)] * 2 if np.isscalar(dst_cap) else [int(dst_cap[0]), int(dst_cap[1])]
        msgs_cap = buf.nbytes // 28 + 1 if msgs_cap is None else int(msgs_cap)
        msgs, info = np.zeros(max(msgs_cap, 1), BAG_MESSAGE_DTYPE), BagInfo()
        ptrs, outs = (C.c_void_p * 2)(), []
        for cam in range(2):
            if device:
                d = C.c_void_p()
                rc = L.esvio_fe_mem_alloc(DEVICE, 16 * max(caps[cam], 1), C.byref(d))
                if rc:
                    raise FrontendError("esvio_fe_mem_alloc rc=%d" % rc)
                outs.append(d)
                ptrs[cam] = d.value
            else:
                outs.append(np.zeros(max(caps[cam], 1), EVENT_DTYPE))
                ptrs[cam] = outs[cam].ctypes.data
        rc = L.esvio_fe_decode_bag(self._hd.h, _p(buf) if buf.nbytes else None, buf.nbytes, int(flags), C.byref(ptrs),
                                   C.byref((C.c_size_t * 2)(*caps)), DEVICE if device else HOST, _p(msgs), msgs_cap, C.byref(info))
        if rc:
            if device:
                for d in outs:
                    L.esvio_fe_mem_free(DEVICE, d)
            e = FrontendError("rc=%d: %s" % (rc, L.esvio_fe_last_error(self._hd.h).decode()))
            e.info = info
            raise e
        k = [int(info.cam[0].events), int(info.cam[1].events)]
        ev = tuple(FilteredEvents(outs[cam], k[cam], None) if device else outs[cam][:k[cam]] for cam in range(2))
        return ev, msgs[:int(info.cam[0].messages + info.cam[1].messages)], info

    def bag_side(self, data, imu_cap=None, flags=0):
        """the sensor_msgs/Imu samples of a chunk of rosbag bytes (esvio_fe_bag_side): the side walker advanced by `data`.
        Returns (imu, BagSideInfo): a numpy IMU_DTYPE array, what MotionCorrection.imu_samples takes.  imu_cap None: what
        the chunk can hold at the most.  A failed call raises FrontendError with `.info`."""
        L = self._hd.L
        buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data)
        imu_cap = buf.nbytes // 296 + 1 if imu_cap is None else int(imu_cap)
        imu, info = np.zeros(max(imu_cap, 1), IMU_DTYPE), BagSideInfo()
        rc = L.esvio_fe_bag_side(self._hd.h, _p(buf) if buf.nbytes else None, buf.nbytes, int(flags), _p(imu), imu_cap, C.byref(info))
        if rc:
            e = FrontendError("rc=%d: %s" % (rc, L.esvio_fe_last_error(self._hd.h).decode()))
            e.info = info
            raise e
        return imu[:int(info.imu)], info

    def bag_set_image_topics(self, left=None, right=None):
        """which topics of a rosbag hold the left and right sensor_msgs/Image messages (esvio_fe_bag_set_image_topics;
        None: none).  Clears the image walker's state only."""
        enc = lambda t: None if t is None else (t if isinstance(t, bytes) else str(t).encode())
        self._hd.check(self._hd.L.esvio_fe_bag_set_image_topics(self._hd.h, enc(left), enc(right)))

    def decode_bag_images(self, data, dst_cap=None, msgs_cap=None, device=False, flags=0):
        """the rosbag image call (esvio_fe_decode_bag_images; include/esvio_fe.h "rosbag images" has the rule): the image
        walker advanced by `data`, host memory, which may end anywhere.  Returns ((left, right), table, BagImageInfo): per
        camera a numpy uint8 array [n, height, width] of gray images, or with device=True a DeviceImages (the caller
        frees it; `.image(k)` is the pointer trackImage(..., device=True) takes); table a numpy BAG_IMAGE_DTYPE array.
        dst_cap None: what the chunk and the bytes that wait can complete at the most; a number or a pair.  A failed
        call raises FrontendError with `.info`."""
        L = self._hd.L
        W, H = self.cfg.width, self.cfg.height
        buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data)
        most = buf.nbytes // (38 + H) + 1  # (a message is 37 bytes and `height` rows of a byte at the least; one may have waited)
        if dst_cap is None:
            dst_cap = most
        caps = [int(dst_cap)] * 2 if np.isscalar(dst_cap) else [int(dst_cap[0]), int(dst_cap[1])]
        msgs_cap = most if msgs_cap is None else int(msgs_cap)
        msgs, info = np.zeros(max(msgs_cap, 1), BAG_IMAGE_DTYPE), BagImageInfo()
        ptrs, outs = (C.c_void_p * 2)(), []
        for cam in range(2):
            if device:
                d = C.c_void_p()
                rc = L.esvio_fe_mem_alloc(DEVICE, W * H * max(caps[cam], 1), C.byref(d))
                if rc:
                    raise FrontendError("esvio_fe_mem_alloc rc=%d" % rc)
                outs.append(d)
                ptrs[cam] = d.value
            else:
                outs.append(np.zeros((max(caps[cam], 1), H, W), np.uint8))
                ptrs[cam] = outs[cam].ctypes.data
        rc = L.esvio_fe_decode_bag_images(self._hd.h, _p(buf) if buf.nbytes else None, buf.nbytes, int(flags), C.byref(ptrs),
                                          C.byref((C.c_size_t * 2)(*caps)), DEVICE if device else HOST, _p(msgs), msgs_cap, C.byref(info))
        if rc:
            if device:
                for d in outs:
                    L.esvio_fe_mem_free(DEVICE, d)
            e = FrontendError("rc=%d: %s" % (rc, L.esvio_fe_last_error(self._hd.h).decode()))
            e.info = info
            raise e
        k = [int(info.cam[0].images), int(info.cam[1].images)]
        img = tuple(DeviceImages(outs[cam], k[cam], W, H) if device else outs[cam][:k[cam]] for cam in range(2))
        return img, msgs[:k[0] + k[1]], info

    def convert_image(self, src, height, width, step, encoding, src_space=HOST, device=False):
        """getImageFromMsg's conversion alone (esvio_fe_convert_image): `src` a numpy uint8 array (host) or a device
        pointer (src_space=DEVICE) whose rows lie `step` bytes apart, encoding ENC_MONO / ENC_BGR / ENC_RGB.  Returns the
        gray image [height, width], or with device=True a DeviceImages of one image (the caller frees it)."""
        L = self._hd.L
        sp = _p(src) if isinstance(src, np.ndarray) else C.c_void_p(int(src))
        if device:
            d = C.c_void_p()
            rc = L.esvio_fe_mem_alloc(DEVICE, max(int(height) * int(width), 1), C.byref(d))
            if rc:
                raise FrontendError("esvio_fe_mem_alloc rc=%d" % rc)
            out, dp = DeviceImages(d, 1, int(width), int(height)), d
        else:
            out = np.zeros((int(height), int(width)), np.uint8)
            dp = _p(out)
        rc = L.esvio_fe_convert_image(self._hd.h, sp, int(src_space), int(height), int(width), int(step), int(encoding), dp, DEVICE if device else HOST)
        if rc:
            if device:
                out.free()
            raise FrontendError("rc=%d: %s" % (rc, L.esvio_fe_last_error(self._hd.h).decode()))
        return out

    def feed_push_bag(self, data, flags=0):
        """append both cameras' events of a chunk of rosbag bytes, left before right (esvio_fe_feed_push_bag; host memory;
        the chunk may end anywhere).  Returns (FeedInfo, FeedInfo); a failed push raises FrontendError with `.info`."""
        buf = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data)
        info = (FeedInfo * 2)()
        self._feed_pushed(self._hd.L.esvio_fe_feed_push_bag(self._hd.h, _p(buf) if buf.nbytes else None, buf.nbytes, int(flags), C.byref(info)), info)
        return info[0], info[1]

    def slice_events(self, cam, ev, frequency=30.0, origin=None, cuts_cap=SLICE_MAX_WINDOWS):
        """the stream-slicing stage (esvio_fe_slice_events; include/esvio_fe.h has the rule): camera `cam`'s slicer
        advanced by `ev` — a numpy EVENT_DTYPE array or a (device_ptr, n) tuple.  origin None: the windows count from the
        camera's first event; else (sec, nsec).  Returns (cuts, SliceInfo): cuts[j] = the index in `ev` of the first event
        behind the j-th window this call closed (numpy uint64, info.closed entries).  A failed call raises FrontendError
        with `.info`; the camera's state is then as it was."""
        ptr, n, space, keep = _events_arg(ev)
        prm, info = SliceParams(frequency, origin), SliceInfo()
        cuts = np.zeros(max(int(cuts_cap), 1), np.uint64)
        rc = self._hd.L.esvio_fe_slice_events(self._hd.h, int(cam), ptr, n, space, C.byref(prm), _p(cuts), int(cuts_cap), C.byref(info))
        if rc:
            e = FrontendError("rc=%d: %s" % (rc, self._hd.L.esvio_fe_last_error(self._hd.h).decode()))
            e.info = info
            raise e
        return cuts[:int(info.closed)], info

    def slice_events_at(self, cam, ev, bounds, cuts_cap=SLICE_MAX_WINDOWS):
        """windows that end at given stamps (esvio_fe_slice_events_at; include/esvio_fe.h has the rule): `bounds` a numpy
        array with `sec` / `nsec` fields (EVENT_DTYPE or TRIGGER_DTYPE records, what decode_triggers returns) or a
        sequence of (sec, nsec) pairs — the ends of the windows from the camera's closed count on, non-decreasing.
        Returns (cuts, SliceInfo) as slice_events does; pass bounds[info.closed:] and newer ones next time."""
        from .events import EVENT_DTYPE
        ptr, n, space, keep = _events_arg(ev)
        if isinstance(bounds, np.ndarray) and bounds.dtype.names and "sec" in bounds.dtype.names:
            sec, nsec = bounds["sec"], bounds["nsec"]
        else:
            pairs = np.asarray(bounds, np.int64).reshape(-1, 2)
            sec, nsec = pairs[:, 0], pairs[:, 1]
        b = np.zeros(len(sec), EVENT_DTYPE)
        b["sec"], b["nsec"] = sec, nsec
        info = SliceInfo()
        cuts = np.zeros(max(int(cuts_cap), 1), np.uint64)
        rc = self._hd.L.esvio_fe_slice_events_at(self._hd.h, int(cam), ptr, n, space, _p(b) if len(b) else None, len(b), _p(cuts),
                                                 int(cuts_cap), C.byref(info))
        if rc:
            e = FrontendError("rc=%d: %s" % (rc, self._hd.L.esvio_fe_last_error(self._hd.h).decode()))
            e.info = info
            raise e
        return cuts[:int(info.closed)], info

    def slice_flush(self, cam):
        """close camera `cam`'s open window, the end of a stream (esvio_fe_slice_flush).  Returns the SliceInfo."""
        info = SliceInfo()
        self._hd.check(self._hd.L.esvio_fe_slice_flush(self._hd.h, int(cam), C.byref(info)))
        return info

    def slice_reset(self):
        """both cameras' slicer states back to the fresh state (esvio_fe_slice_reset)"""
        self._hd.check(self._hd.L.esvio_fe_slice_reset(self._hd.h))

    def feed_open(self, frequency=30.0, origin=None, params=None):
        """open the handle's feed (esvio_fe_feed_open; include/esvio_fe.h): chunks pushed per camera are cut into windows
        of 1 / frequency seconds counted from `origin` ((sec, nsec); None: the first left record), through the filter
        `params` (a FilterParams) if given"""
        prm = SliceParams(frequency, origin)
        self._hd.check(self._hd.L.esvio_fe_feed_open(self._hd.h, C.byref(prm), C.byref(params) if params is not None else None))

    def _feed_pushed(self, rc, info):
        if rc:
            e = FrontendError("rc=%d: %s" % (rc, self._hd.L.esvio_fe_last_error(self._hd.h).decode()))
            e.info = info
            raise e
        return info

    def feed_push_events(self, cam, ev):
        """append a chunk of records — a numpy EVENT_DTYPE array or a (device_ptr, n) tuple — to camera `cam`'s stream.
        Returns the FeedInfo; a failed push raises FrontendError with `.info`."""
        ptr, n, space, keep = _events_arg(ev)
        info = FeedInfo()
        return self._feed_pushed(self._hd.L.esvio_fe_feed_push_events(self._hd.h, int(cam), ptr, n, space, C.byref(info)), info)

    def feed_push_fields(self, cam, fields, src_space=HOST):
        """append a chunk given as events.EventFields (`src_space` says where the fields lie)"""
        d, info = fields_desc(fields), FeedInfo()
        return self._feed_pushed(self._hd.L.esvio_fe_feed_push_fields(self._hd.h, int(cam), C.byref(d), fields.n, src_space, C.byref(info)), info)

    def feed_push_raw(self, cam, fmt, words, t_offset_us=0):
        """append a chunk of raw words (a contiguous numpy array — its bytes are the stream — or a (device_ptr, n_bytes)
        tuple) of format RAW_EVT2 / RAW_EVT3; the chunk may end anywhere"""
        if isinstance(words, tuple):
            ptr, nbytes, space = C.c_void_p(words[0]), int(words[1]), DEVICE
        else:
            words = np.ascontiguousarray(words)
            ptr, nbytes, space = _p(words), words.nbytes, HOST
        info = FeedInfo()
        return self._feed_pushed(self._hd.L.esvio_fe_feed_push_raw(self._hd.h, int(cam), int(fmt), ptr, nbytes, space, int(t_offset_us),
                                                                   C.byref(info)), info)

    def feed_push_text(self, cam, order, time, data, flags=0, t_offset_ns=0):
        """append the event lines of a chunk of a text event file (as decode_text takes it); the chunk may end anywhere"""
        ptr, nbytes, space, keep = _text_src(data)
        fmt, info = TextFormat(int(order), int(time), int(flags), 0), FeedInfo()
        return self._feed_pushed(self._hd.L.esvio_fe_feed_push_text(self._hd.h, int(cam), C.byref(fmt), ptr, nbytes, space,
                                                                    int(t_offset_ns), C.byref(info)), info)

    def feed_peek(self):
        """the oldest window closed in both cameras and not yet tracked, as a FeedWindow (.index, .end_sec / .end_nsec =
        E_k, .count), or None"""
        w = FeedWindow()
        self._hd.check(self._hd.L.esvio_fe_feed_peek(self._hd.h, C.byref(w)))
        return w if w.ready else None

    def feed_track(self, pub=True, measurements=None, copy=True):
        """track the window feed_peek shows (esvio_fe_feed_track).  Returns the BatchInfo: .kept, .cur_time, .tracked (0:
        the left window was empty, the result members are the previous call's)."""
        info = BatchInfo()
        self._hd.check(self._hd.L.esvio_fe_feed_track(self._hd.h, int(pub), C.byref(measurements) if measurements is not None else None,
                                                      C.byref(self._tr), C.byref(info)))
        if info.tracked:
            self._take(copy)
        return info

    def feed_close(self):
        """close the handle's feed (esvio_fe_feed_close): what it still holds is dropped"""
        self._hd.check(self._hd.L.esvio_fe_feed_close(self._hd.h))

    def filter_reset(self):
        """every stamp plane of the background-activity filter back to `none` (esvio_fe_filter_reset)"""
        self._hd.check(self._hd.L.esvio_fe_filter_reset(self._hd.h))

    def trackEventFiltered(self, left, right, window_ns, min_support=1, pub=True, copy=True):
        """filter both cameras' batches, then trackEvent on the kept records at the stamp of the last kept left
        event (esvio_fe_track_event_filtered).  Returns (kept, cur_time): kept = (left, right) counts; with
        kept[0] == 0 nothing was tracked, cur_time is None and the result members are the previous call's."""
        pl, nl, sl, k1 = _events_arg(left)
        pr, nr, sr, k2 = _events_arg(right)
        assert sl == sr
        kept = (C.c_uint64 * 2)()
        t = C.c_double(0.0)
        self._hd.check(self._hd.L.esvio_fe_track_event_filtered(
            self._hd.h, pl, nl, pr, nr, sl, int(window_ns), int(min_support), int(pub), C.byref(self._tr),
            C.byref(kept), C.byref(t)))
        if kept[0]:
            self._take(copy)
        return (int(kept[0]), int(kept[1])), (t.value if kept[0] else None)

    _LEFT = frozenset(("ids", "track_cnt", "cur_pts", "cur_un_pts", "pts_velocity"))
    _RIGHT = frozenset(("ids_right", "cur_right_pts", "cur_un_right_pts", "right_pts_velocity"))
    _RESULTS = tuple(sorted(_LEFT | _RIGHT))

    def _take(self, copy):
        """the result members (.ids, .cur_pts, ...) are cut out of the call's output buffers when they are READ
        (__getattr__ below), not after every call: a replaying caller that looks at none of them pays nothing for
        them — nine slices and attribute stores were ~3 us of Python between two track calls"""
        d = self.__dict__
        for k in self._RESULTS:
            d.pop(k, None)
        self._copy = copy
        return self

    def __getattr__(self, name):  # (only reached when the attribute is not set: a result member not read yet)
        if name in FeatureTracker._LEFT:
            v = self._bufs[name][:self._tr.n_left]
        elif name in FeatureTracker._RIGHT:
            v = self._bufs[name][:self._tr.n_right]
        else:
            raise AttributeError(name)
        if self._copy:
            v = v.copy()
        self.__dict__[name] = v
        return v

    def trackImage(self, cur_time, img_left, img_right, PUB_THIS_FRAME=True, copy=True, device=False):
        """FeatureTracker::trackImage (feature_tracker.cpp:164-338); the handle's width/height/
        max_cnt/min_dist are the image camera's COL/ROW/MAX_CNT_IMG/MIN_DIST_IMG.  device=True: img_left and img_right
        are pointers to dense gray images in device memory (esvio_fe_track_image_space; DeviceImages.image(k))"""
        if device:
            self._hd.check(self._hd.L.esvio_fe_track_image_space(
                self._hd.h, float(cur_time), C.c_void_p(int(img_left)), None if img_right is None else C.c_void_p(int(img_right)), DEVICE,
                int(PUB_THIS_FRAME), C.byref(self._tr)))
            return self._take(copy)
        il = np.ascontiguousarray(img_left, np.uint8)
        assert il.shape == (self.cfg.height, self.cfg.width)
        ir = None
        if img_right is not None:
            ir = np.ascontiguousarray(img_right, np.uint8)
            assert ir.shape == il.shape
        self._hd.check(self._hd.L.esvio_fe_track_image(
            self._hd.h, float(cur_time), _p(il), None if ir is None else _p(ir), int(PUB_THIS_FRAME),
            C.byref(self._tr)))
        return self._take(copy)

    def goodFeaturesToTrack(self, image, maxCorners, qualityLevel=0.01, minDistance=30, mask=None,
                            want_eig=False):
        """cv::goodFeaturesToTrack(image, maxCorners, qualityLevel, minDistance, mask) with
        trackImage's defaults (feature_tracker.cpp:228)"""
        img = np.ascontiguousarray(image, np.uint8)
        assert img.shape == (self.cfg.height, self.cfg.width)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        out = np.zeros((max(int(maxCorners), 1), 2), np.float32)
        eig = np.zeros(img.shape, np.float32) if want_eig else None
        n = C.c_int32()
        self._hd.check(self._hd.L.esvio_fe_good_features_to_track(
            self._hd.h, _p(img), int(maxCorners), float(qualityLevel), float(minDistance),
            None if m is None else _p(m), _p(out), C.byref(n), None if eig is None else _p(eig)))
        return (out[:n.value].copy(), eig) if want_eig else out[:n.value].copy()

    def set_lazy_new_stereo(self, on=True):
        """throughput option: published frames do not wait for the stereo LK of the corners they have
        just detected; finish() (or the next call) completes the right-camera vectors"""
        self._hd.check(self._hd.L.esvio_fe_set_lazy_new_stereo(self._hd.h, int(bool(on))))

    def set_host_threads(self, threads):
        """host threads for rejectWithF_event's RANSAC (results do not depend on the count)"""
        self._hd.check(self._hd.L.esvio_fe_set_host_threads(self._hd.h, int(threads)))

    def set_launch_thread(self, on=True):
        """replay mode: a thread of the handle issues the announced batches' prefetch launches"""
        self._hd.check(self._hd.L.esvio_fe_set_launch_thread(self._hd.h, int(bool(on))))

    def finish(self, copy=True):
        """complete a lazily returned frame and refresh the result members"""
        self._hd.check(self._hd.L.esvio_fe_finish(self._hd.h, C.byref(self._tr)))
        return self._take(copy)

    def pack_track_records(self, out=None):
        """node:273-329 packing of the current results into a (2*max_cnt, 8) float32 block
        (padding rows have id -1); `out` may be a preallocated (e.g. pinned) array"""
        if out is None:
            out = np.empty((2 * self.cfg.max_cnt, 8), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == 16 * self.cfg.max_cnt
        n = C.c_int32()
        self._hd.check(self._hd.L.esvio_fe_pack_track_records(self._hd.h, _p(out), C.byref(n)))
        return out

    def set_next_batch(self, next_cur_time, event_left, event_right, PUB_NEXT_FRAME=False, measurements=None):
        """announce the batch of the FOLLOWING trackEvent call (throughput / replay mode);
        PUB_NEXT_FRAME is the PUB_THIS_FRAME that call is expected to carry (a hint);
        `measurements`: the esvio_fe_motion that call will pass (motion-compensated overload)"""
        pl, nl, sl, k1 = _events_arg(event_left)
        pr, nr, sr, k2 = _events_arg(event_right)
        assert sl == sr
        # host arrays must outlive the prefetch (up to six announced + the one being tracked)
        self._next_keep = (getattr(self, "_next_keep", []) + [(k1, k2)])[-8:]
        if measurements is None:
            self._hd.check(self._hd.L.esvio_fe_set_next_batch(self._hd.h, float(next_cur_time), pl, nl,
                                                              pr, nr, sl, int(bool(PUB_NEXT_FRAME))))
        else:
            self._hd.check(self._hd.L.esvio_fe_set_next_batch_mc(self._hd.h, float(next_cur_time), pl, nl, pr, nr, sl,
                                                                 int(bool(PUB_NEXT_FRAME)), C.byref(measurements)))

    def reset(self):
        self._hd.check(self._hd.L.esvio_fe_reset(self._hd.h))

    def reserve(self, max_left, max_right, host_batches=False):
        """size every event-proportional buffer for batches of up to max_left + max_right events now, so
        that no later call below that size allocates (esvio_fe_reserve)"""
        self._hd.check(self._hd.L.esvio_fe_reserve(self._hd.h, int(max_left), int(max_right), int(bool(host_batches))))

    def latency_stats(self, reset=False):
        """wall time of the trackEvent calls since the last reset as the calling thread saw them: count,
        mean / p50 / p99 / max [ms], and for the slowest call its index, its phases [ms], the CPUs it began
        and ended on, involuntary context switches and allocations inside it"""
        o = Latency()
        L = self._hd.L
        self._hd.check(L.esvio_fe_latency_stats(self._hd.h, C.byref(o), int(bool(reset))))
        phases = {L.esvio_fe_latency_phase_name(k).decode(): round(o.max_phase_ms[k], 4)
                  for k in range(LATENCY_PHASES) if o.max_phase_ms[k] > 0.0005}
        return dict(calls=int(o.calls), mean_ms=o.mean_ms, p50_ms=o.p50_ms, p99_ms=o.p99_ms, max_ms=o.max_ms,
                    max_call=int(o.max_call), max_published=bool(o.max_published),
                    max_cpu=(int(o.max_cpu_begin), int(o.max_cpu_end)), max_invol_switches=int(o.max_invol_switches),
                    max_allocs=int(o.max_allocs), max_phase_ms=phases, allocs=int(o.allocs),
                    invol_switches=int(o.invol_switches))

    def latency_recent(self, n):
        """the latest n (<= 256) track calls, oldest first: (call, published, begin_ms, ms, {phase: ms})"""
        L = self._hd.L
        names = [L.esvio_fe_latency_phase_name(k).decode() for k in range(LATENCY_PHASES)]
        out = []
        for back in range(n - 1, -1, -1):
            o = LatencyCall()
            if L.esvio_fe_latency_recent(self._hd.h, back, C.byref(o)) != 0:
                continue
            out.append((int(o.call), bool(o.published), o.begin_ms, o.ms,
                        {names[k]: o.phase_ms[k] for k in range(LATENCY_PHASES) if o.phase_ms[k] > 0.0005}))
        return out

    def debug_inject(self, mask):
        """make device-side waits expire on demand (FAULT_TICKET | FAULT_LOOKBACK | FAULT_SPECULATIVE |
        FAULT_CHAINED; 0: normal bounds), or replay mode's lazy completions always happen at their latest point
        (FAULT_LAZY_LATE)"""
        self._hd.check(self._hd.L.esvio_fe_debug_inject(self._hd.h, int(mask)))

    def staging_counters(self):
        """host batches staged / bytes / chunks that crossed PCIe packed to 8 B per event / chunks of such batches sent raw"""
        out = (C.c_uint64 * 4)()
        self._hd.check(self._hd.L.esvio_fe_staging_counters(self._hd.h, out))
        return dict(batches=out[0], bytes=out[1], chunks_packed=out[2], chunks_raw=out[3])

    def debug_counters(self):
        out = (C.c_uint64 * 4)()
        self._hd.check(self._hd.L.esvio_fe_debug_counters(self._hd.h, out))
        return dict(spec_redone=out[0], chain_redone=out[1], chain_launched=out[2], chain_used=out[3])

    def plain_call_counters(self):
        out = (C.c_uint64 * 4)()
        self._hd.check(self._hd.L.esvio_fe_plain_call_counters(self._hd.h, out))
        return dict(plain_calls=out[0], split_by_camera=out[1], stereo_chained=out[2], chained_redone=out[3])

    # ---- the handle's own RCCL communicator: asynchronous exchange of the track records
    def comm_init(self, unique_id, rank, world):
        """unique_id: the 128 bytes of comm_unique_id() made on rank 0"""
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._hd.check(self._hd.L.esvio_fe_comm_init(self._hd.h, buf, int(rank), int(world)))
        self._x_world = int(world)

    def set_auto_exchange(self, on=True):
        self._hd.check(self._hd.L.esvio_fe_set_auto_exchange(self._hd.h, int(bool(on))))

    def exchange_begin(self):
        self._hd.check(self._hd.L.esvio_fe_exchange_begin(self._hd.h))

    def exchange_end(self, want=True):
        """wait for the latest exchange_begin; -> (world, 2*max_cnt, 8) float32, or None"""
        out = np.empty((self._x_world, 2 * self.cfg.max_cnt, 8), np.float32) if want else None
        self._hd.check(self._hd.L.esvio_fe_exchange_end(self._hd.h, _p(out)))
        return out

    def device_memory(self):
        """(free, total) bytes of the handle's device"""
        f, t = C.c_size_t(0), C.c_size_t(0)
        self._hd.check(self._hd.L.esvio_fe_device_memory(self._hd.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    # ---- one stream time-sliced across GPUs (esvio_fe_sae_slice_*); plane sets are numpy float64
    # arrays (host) or (device_ptr, n_sets) tuples
    def sae_plane_doubles(self):
        return int(self._hd.L.esvio_fe_sae_plane_doubles(self._hd.h))

    @staticmethod
    def _planes_arg(a):
        if isinstance(a, tuple):
            return C.c_void_p(a[0]), DEVICE
        return _p(a), HOST

    def sae_slice_last(self, event_left, event_right, out):
        pl, nl, sl, k1 = _events_arg(event_left)
        pr, nr, sr, k2 = _events_arg(event_right)
        assert sl == sr
        po, so = self._planes_arg(out)
        self._hd.check(self._hd.L.esvio_fe_sae_slice_last(self._hd.h, pl, nl, pr, nr, sl, po, so))

    def sae_slice_apply(self, event_left, event_right, last_before, n_before, s_out):
        pl, nl, sl, k1 = _events_arg(event_left)
        pr, nr, sr, k2 = _events_arg(event_right)
        assert sl == sr
        pi, si = self._planes_arg(last_before) if n_before else (None, HOST)
        po, so = self._planes_arg(s_out)
        self._hd.check(self._hd.L.esvio_fe_sae_slice_apply(self._hd.h, pl, nl, pr, nr, sl, pi, int(n_before),
                                                          si, po, so))

    def sae_slice_commit(self, last_all, s_all, n_slices):
        pa, sa = self._planes_arg(last_all)
        pb, sb = self._planes_arg(s_all)
        assert sa == sb
        self._hd.check(self._hd.L.esvio_fe_sae_slice_commit(self._hd.h, pa, pb, int(n_slices), sa))

    def gettimesurface(self, cam=0):
        out = np.empty((self.cfg.height, self.cfg.width), np.uint8)
        self._hd.check(self._hd.L.esvio_fe_get_time_surface(self._hd.h, cam, _p(out)))
        return out

    def fast_corners(self, img=None, cam=0, arc=10, barrier=20, nonmax=True, capacity=None, want_count=False):
        """FAST-9/10 corners (the reference's vendored fast::fast_corner_detect_9/_10, fast_corner_score_10,
        fast_nonmax_3x3) of the current time surface of `cam` (img None), of a numpy (H,W) u8 image or of a
        device image given as int pointer -> (xy int16[n,2] in raster order, score int32[n] or None for arc 9).
        capacity: room for that many corners only (the first ones); default: call again if the first guess
        was too small.  want_count: also return (n_out, n_detected), the full counts after / before non-max."""
        hd = self._hd
        if img is None:
            ptr, space, keep = None, HOST, None
        elif isinstance(img, np.ndarray):
            keep = np.ascontiguousarray(img, np.uint8)
            if keep.shape != (self.cfg.height, self.cfg.width):
                raise ValueError("image must be (height, width) of the handle")
            ptr, space = _p(keep), HOST
        else:
            ptr, space, keep = C.c_void_p(int(img)), DEVICE, None
        cap = 4096 if capacity is None else int(capacity)
        n, nd = C.c_int32(0), C.c_int32(0)
        while True:
            xy = np.empty((max(cap, 1), 2), np.int16)
            sc = np.empty(max(cap, 1), np.int32) if arc == 10 else None
            hd.check(hd.L.esvio_fe_fast_corners(hd.h, cam, ptr, space, arc, barrier, 1 if nonmax else 0, _p(xy),
                                                _p(sc) if sc is not None else None, cap, C.byref(n), C.byref(nd)))
            if capacity is not None or n.value <= cap:
                break
            cap = n.value
        k = min(n.value, cap)
        out = (xy[:k].copy(), sc[:k].copy() if sc is not None else None)
        return out + ((n.value, nd.value),) if want_count else out

    def set_detector(self, detector, barrier=20):
        """where trackEvent takes a published frame's new corners from: DETECT_ARC (the reference, the default) or
        DETECT_FAST — FAST-10 + score + non-max on the raw left time surface at `barrier`, ordered by score, then
        the same greedy min_dist scan (include/esvio_fe.h).  Not while batches are announced; survives reset()."""
        self._hd.check(self._hd.L.esvio_fe_set_detector(self._hd.h, int(detector), int(barrier)))

    def features_to_track_fast(self, img=None, barrier=20, maxCorners=None, mask=None, want_count=False):
        """the DETECT_FAST selection for one image (esvio_fe_features_to_track_fast): the current raw left time
        surface (img None), a numpy (H,W) u8 image or a device image given as int pointer; mask: (H,W) u8,
        255 = blocked -> (xy float32[n,2], score int32[n]) in the order of acceptance; want_count: also the number of
        FAST corners after non-max, before any mask or threshold test"""
        hd = self._hd
        if img is None:
            ptr, space, keep = None, HOST, None
        elif isinstance(img, np.ndarray):
            keep = np.ascontiguousarray(img, np.uint8)
            if keep.shape != (self.cfg.height, self.cfg.width):
                raise ValueError("image must be (height, width) of the handle")
            ptr, space = _p(keep), HOST
        else:
            ptr, space, keep = C.c_void_p(int(img)), DEVICE, None
        m = self.cfg.max_cnt if maxCorners is None else int(maxCorners)
        xy = np.zeros((max(m, 1), 2), np.float32)
        sc = np.zeros(max(m, 1), np.int32)
        k, nc = C.c_int32(0), C.c_int32(0)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        hd.check(hd.L.esvio_fe_features_to_track_fast(hd.h, ptr, space, int(barrier), m, _p(mk), _p(xy), _p(sc),
                                                      C.byref(k), C.byref(nc)))
        out = (xy[:k.value].copy(), sc[:k.value].copy())
        return out + (nc.value,) if want_count else out

    # ---- loop-closure keyframes (esvio_fe_kf_*; include/esvio_fe.h "keyframes" has the rules)
    def _kf_image(self, img):
        """None (the handle's plane), a numpy (H,W) u8 image or a device image given as int pointer -> (ptr, space, keep)"""
        if img is None:
            return None, HOST, None
        if isinstance(img, np.ndarray):
            keep = np.ascontiguousarray(img, np.uint8)
            if keep.shape != (self.cfg.height, self.cfg.width):
                raise ValueError("image must be (height, width) of the handle")
            return _p(keep), HOST, keep
        return C.c_void_p(int(img)), DEVICE, None

    def kf_set_pattern(self, x1, y1, x2, y2):
        """the BRIEF pattern (esvio_fe_kf_set_pattern): four lists of 256 integers, as parse_brief_pattern returns
        them; survives reset()"""
        a = [np.ascontiguousarray(v, np.int32) for v in (x1, y1, x2, y2)]
        n = len(a[0])
        if any(len(v) != n for v in a):
            raise ValueError("the four pattern lists differ in length")
        self._hd.check(self._hd.L.esvio_fe_kf_set_pattern(self._hd.h, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), n))

    def kf_blur(self, img=None, dst=None):
        """cv::GaussianBlur(9x9, sigma 2) of the image (esvio_fe_kf_blur) -> numpy (H,W) u8, or into the device buffer
        given as int pointer `dst`"""
        ptr, space, keep = self._kf_image(img)
        if dst is None:
            out = np.empty((self.cfg.height, self.cfg.width), np.uint8)
            self._hd.check(self._hd.L.esvio_fe_kf_blur(self._hd.h, ptr, space, _p(out), HOST))
            return out
        self._hd.check(self._hd.L.esvio_fe_kf_blur(self._hd.h, ptr, space, C.c_void_p(int(dst)), DEVICE))
        return None

    def kf_fast(self, img=None, threshold=20, capacity=None, want_count=False):
        """cv::FAST(img, kps, threshold, true) (esvio_fe_kf_fast) -> (xy float32[n,2] in raster order, score int32[n]);
        capacity: room for that many corners only (the first ones); want_count: also (n_out, n_detected)"""
        hd = self._hd
        ptr, space, keep = self._kf_image(img)
        cap = 4096 if capacity is None else int(capacity)
        n, nd = C.c_int32(0), C.c_int32(0)
        while True:
            xy = np.empty((max(cap, 1), 2), np.float32)
            sc = np.empty(max(cap, 1), np.int32)
            hd.check(hd.L.esvio_fe_kf_fast(hd.h, ptr, space, int(threshold), _p(xy), _p(sc), cap, C.byref(n), C.byref(nd)))
            if capacity is not None or n.value <= cap:
                break
            cap = n.value
        k = min(n.value, cap)
        out = (xy[:k].copy(), sc[:k].copy())
        return out + ((n.value, nd.value),) if want_count else out

    def kf_brief(self, blurred, pts, desc=None):
        """BRIEF::compute(treat_image = false) at the (x, y) float pairs `pts` on the blurred image (numpy or device
        pointer; esvio_fe_kf_brief) -> uint32[n,8], or into the device buffer given as int pointer `desc`"""
        ptr, space, keep = self._kf_image(blurred)
        p = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        n = len(p)
        if desc is None:
            out = np.zeros((n, 8), np.uint32)
            self._hd.check(self._hd.L.esvio_fe_kf_brief(self._hd.h, ptr, space, _p(p) if n else None, n, _p(out) if n else None, HOST))
            return out
        self._hd.check(self._hd.L.esvio_fe_kf_brief(self._hd.h, ptr, space, _p(p) if n else None, n, C.c_void_p(int(desc)), DEVICE))
        return None

    def kf_match(self, query, train, nq=None, nt=None):
        """searchInAera for every query (esvio_fe_kf_match): numpy uint32[n,8] arrays, or device pointers (int) with
        nq / nt -> (idx int32[nq], dist int32[nq], status uint8[nq])"""
        if isinstance(query, np.ndarray):
            q = np.ascontiguousarray(query, np.uint32).reshape(-1, 8)
            t = np.ascontiguousarray(train, np.uint32).reshape(-1, 8)
            nq, nt, space = len(q), len(t), HOST
            qp, tp = (_p(q) if nq else None), (_p(t) if nt else None)
        else:
            space, qp, tp = DEVICE, C.c_void_p(int(query)), C.c_void_p(int(train))
        idx, dist, st = np.zeros(max(nq, 1), np.int32), np.zeros(max(nq, 1), np.int32), np.zeros(max(nq, 1), np.uint8)
        self._hd.check(self._hd.L.esvio_fe_kf_match(self._hd.h, qp, int(nq), tp, int(nt), space, _p(idx), _p(dist), _p(st)))
        return idx[:nq], dist[:nq], st[:nq]

    def keyframe_describe(self, img=None, window_pts=(), cam=0, fast_threshold=20, kp_capacity=None, device_desc=None):
        """KeyFrame::KeyFrame's computeWindowBRIEFPoint + computeBRIEFPoint (esvio_fe_kf_describe) -> dict(window_desc,
        kp_xy, kp_score, kp_norm, kp_desc, n_kp, n_detected).  device_desc: (window_desc_ptr, kp_desc_ptr) device
        buffers (int) that take the descriptors instead of the returned arrays (then None in the dict)."""
        hd = self._hd
        ptr, space, keep = self._kf_image(img)
        w = np.ascontiguousarray(window_pts, np.float32).reshape(-1, 2)
        nw = len(w)
        cap = 4096 if kp_capacity is None else int(kp_capacity)
        while True:
            m = max(cap, 1)
            o = KfOut()
            wd = np.zeros((max(nw, 1), 8), np.uint32)
            kxy, ksc, knorm = np.zeros((m, 2), np.float32), np.zeros(m, np.int32), np.zeros((m, 2), np.float32)
            kd = np.zeros((m, 8), np.uint32)
            if device_desc is None:
                o.window_desc, o.kp_desc, o.desc_space = wd.ctypes.data, kd.ctypes.data, HOST
            else:
                o.window_desc, o.kp_desc, o.desc_space = int(device_desc[0]), int(device_desc[1]), DEVICE
            o.kp_xy, o.kp_score, o.kp_norm, o.kp_capacity = kxy.ctypes.data, ksc.ctypes.data, knorm.ctypes.data, cap
            hd.check(hd.L.esvio_fe_kf_describe(hd.h, int(cam), ptr, space, _p(w) if nw else None, nw, int(fast_threshold), C.byref(o)))
            if kp_capacity is not None or o.n_kp <= cap:
                break
            cap = o.n_kp
        k = min(o.n_kp, cap)
        host = device_desc is None
        return dict(window_desc=wd[:nw] if host else None, kp_xy=kxy[:k], kp_score=ksc[:k], kp_norm=knorm[:k],
                    kp_desc=kd[:k] if host else None, n_kp=int(o.n_kp), n_detected=int(o.n_detected))

    def kf_kernel_stats(self):
        """the keyframe stage's own kernel table (esvio_fe_kf_kernel_*): name -> dict(ms, launches, alg_bytes)"""
        L = self._hd.L
        out = {}
        for k in range(L.esvio_fe_kf_kernel_count()):
            ms, n, b = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
            self._hd.check(L.esvio_fe_kf_kernel_stats(self._hd.h, k, C.byref(ms), C.byref(n), C.byref(b)))
            out[L.esvio_fe_kf_kernel_name(k).decode()] = dict(ms=ms.value, launches=n.value, alg_bytes=b.value)
        return out

    # ---- loop detection (esvio_fe_bow_*; include/esvio_fe.h "loop detection" has the rules)
    def _bow_desc(self, desc, n):
        """numpy uint32[n,8] descriptors, or a device pointer (int) with n -> (ptr, n, space, keep)"""
        if isinstance(desc, np.ndarray):
            keep = np.ascontiguousarray(desc, np.uint32).reshape(-1, 8)
            return (_p(keep) if len(keep) else None), len(keep), HOST, keep
        return C.c_void_p(int(desc)), int(n), DEVICE, None

    def bow_set_vocabulary(self, data):
        """the vocabulary file's bytes (esvio_fe_bow_set_vocabulary); survives reset()"""
        buf = bytes(data)
        self._hd.check(self._hd.L.esvio_fe_bow_set_vocabulary(self._hd.h, buf, len(buf)))

    def bow_transform(self, desc, n=None, bow_cap=None):
        """W and T (esvio_fe_bow_transform) -> dict(word int32[n], weight float64[n], bow_word uint32[m], bow_value
        float64[m], n_bow); bow_cap: room for that many pairs only (n_bow is the full count)"""
        ptr, n, space, keep = self._bow_desc(desc, n)
        cap = n if bow_cap is None else int(bow_cap)
        word, weight = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float64)
        bw, bv, m = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.float64), C.c_int32(0)
        self._hd.check(self._hd.L.esvio_fe_bow_transform(self._hd.h, ptr, n, space, _p(word), _p(weight), _p(bw), _p(bv), cap, C.byref(m)))
        k = min(m.value, cap)
        return dict(word=word[:n], weight=weight[:n], bow_word=bw[:k], bow_value=bv[:k], n_bow=m.value)

    def bow_add(self, desc, n=None):
        """db.add(desc) (esvio_fe_bow_add) -> the new entry's id"""
        ptr, n, space, keep = self._bow_desc(desc, n)
        e = C.c_int32(-1)
        self._hd.check(self._hd.L.esvio_fe_bow_add(self._hd.h, ptr, n, space, C.byref(e)))
        return e.value

    def bow_query(self, desc, max_results=BOW_LOOP_RESULTS, max_id=-1, n=None):
        """db.query(desc, ret, max_results, max_id) (esvio_fe_bow_query) -> [(id, score), ...]"""
        ptr, n, space, keep = self._bow_desc(desc, n)
        res, k = (BowResult * BOW_MAX_RESULTS)(), C.c_int32(0)
        self._hd.check(self._hd.L.esvio_fe_bow_query(self._hd.h, ptr, n, space, int(max_results), int(max_id), res, C.byref(k)))
        return [(res[j].id, res[j].score) for j in range(k.value)]

    def detect_loop(self, desc, frame_index, n=None):
        """PoseGraph::detectLoop's query, add and decision (esvio_fe_bow_detect_loop) -> (loop index or -1, [(id, score), ...])"""
        ptr, n, space, keep = self._bow_desc(desc, n)
        res, k, m = (BowResult * BOW_LOOP_RESULTS)(), C.c_int32(0), C.c_int32(-1)
        self._hd.check(self._hd.L.esvio_fe_bow_detect_loop(self._hd.h, ptr, n, space, int(frame_index), C.byref(m), res, C.byref(k)))
        return m.value, [(res[j].id, res[j].score) for j in range(k.value)]

    def bow_scores(self, desc, max_id=-1, n=None):
        """the raw sums of a query (esvio_fe_bow_scores, a test tap) -> (score float64[entries], present bool[entries])"""
        ptr, n, space, keep = self._bow_desc(desc, n)
        N = self.bow_entries()
        sc, pr = np.zeros(max(N, 1), np.float64), np.zeros(max(N, 1), np.uint8)
        self._hd.check(self._hd.L.esvio_fe_bow_scores(self._hd.h, ptr, n, space, int(max_id), _p(sc), _p(pr)))
        return sc[:N], pr[:N].astype(bool)

    def bow_entries(self):
        return self._hd.L.esvio_fe_bow_entries(self._hd.h)

    def bow_clear(self):
        self._hd.check(self._hd.L.esvio_fe_bow_clear(self._hd.h))

    def bow_reserve(self, entries, words):
        self._hd.check(self._hd.L.esvio_fe_bow_reserve(self._hd.h, int(entries), int(words)))

    def bow_kernel_stats(self):
        """loop detection's own kernel table (esvio_fe_bow_kernel_*): name -> dict(ms, launches, alg_bytes)"""
        L = self._hd.L
        out = {}
        for k in range(L.esvio_fe_bow_kernel_count()):
            ms, n, b = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
            self._hd.check(L.esvio_fe_bow_kernel_stats(self._hd.h, k, C.byref(ms), C.byref(n), C.byref(b)))
            out[L.esvio_fe_bow_kernel_name(k).decode()] = dict(ms=ms.value, launches=n.value, alg_bytes=b.value)
        return out

    # ---- creating a vocabulary (esvio_fe_bow_create_*; include/esvio_fe.h "C, creating a vocabulary" has the rule)
    def bow_create_vocabulary(self, desc, doc_offsets, k, L, weighting=0, scoring=0, seed=0, max_passes=0, n=None, check=True):
        """esvio_fe_bow_create_vocabulary -> (return code, dict of the info struct); desc as _bow_desc takes it,
        doc_offsets n_docs + 1 ascending offsets.  check: raise on a non-zero return code"""
        ptr, n, space, keep = self._bow_desc(desc, n)
        off = np.ascontiguousarray(doc_offsets, np.int64)
        par = BowCreateParams(int(k), int(L), int(weighting), int(scoring), int(max_passes), 0, int(seed) & 0xffffffffffffffff)
        info = BowCreateInfo()
        rc = self._hd.L.esvio_fe_bow_create_vocabulary(self._hd.h, ptr, n, space, _p(off), len(off) - 1, C.byref(par), C.byref(info))
        if check:
            self._hd.check(rc)
        out = {f: getattr(info, f) for f, _ in BowCreateInfo._fields_ if f != "message"}
        out["message"] = info.message.decode()
        return rc, out

    def bow_get_created(self, n_bytes):
        """the file image of the last successful create (esvio_fe_bow_get_created); n_bytes: info's `bytes`"""
        buf = np.empty(max(int(n_bytes), 1), np.uint8)
        self._hd.check(self._hd.L.esvio_fe_bow_get_created(self._hd.h, _p(buf), int(n_bytes)))
        return buf[:int(n_bytes)].tobytes()

    def bow_create_pick(self, min_dist, seg_off, cut_d):
        """C2's pick alone on the device (esvio_fe_bow_create_pick, a test tap) -> uint32[n_seg] ranks"""
        md = np.ascontiguousarray(min_dist, np.uint32)
        so = np.ascontiguousarray(seg_off, np.uint32)
        cd = np.ascontiguousarray(cut_d, np.float64)
        out = np.zeros(len(cd), np.uint32)
        self._hd.check(self._hd.L.esvio_fe_bow_create_pick(self._hd.h, _p(md), len(md), _p(so), len(so) - 1, _p(cd), _p(out)))
        return out

    def sort_pairs(self, keys, vals, passes, bits, n_dev=-1, fill_keys=0, fill_vals=0):
        """the shared stable sort alone (esvio_fe_sort_pairs, a test tap): `passes` passes of `bits` bits over the low bits of
        keys, in device memory of the call's own; n_dev >= 0: passed as the device-side count.  fill_keys / fill_vals: what
        both device buffers hold where no pass writes.  -> (rc, keys, vals, err, tickets[passes])"""
        k = np.ascontiguousarray(keys, np.uint32)
        v = np.ascontiguousarray(vals, np.uint32)
        assert k.shape == v.shape and k.ndim == 1
        ok = np.full(max(len(k), 1), fill_keys, np.uint32)
        ov = np.full(max(len(k), 1), fill_vals, np.uint32)
        err = C.c_int32(-1)
        tickets = np.full(max(int(passes), 1), 0xffffffff, np.uint32)
        rc = self._hd.L.esvio_fe_sort_pairs(self._hd.h, _p(k), _p(v), len(k), int(passes), int(bits), int(n_dev), _p(ok), _p(ov),
                                            C.byref(err), _p(tickets))
        return rc, ok[:len(k)], ov[:len(k)], err.value, tickets

    def bow_create_kernel_stats(self):
        """vocabulary creation's own kernel table (esvio_fe_bow_create_kernel_*): name -> dict(ms, launches, alg_bytes)"""
        L = self._hd.L
        out = {}
        for k in range(L.esvio_fe_bow_create_kernel_count()):
            ms, n, b = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
            self._hd.check(L.esvio_fe_bow_create_kernel_stats(self._hd.h, k, C.byref(ms), C.byref(n), C.byref(b)))
            out[L.esvio_fe_bow_create_kernel_name(k).decode()] = dict(ms=ms.value, launches=n.value, alg_bytes=b.value)
        return out

    # ---- camera split (right camera on another GPU)
    def export_image(self, cam, dst=None):
        """current image of `cam` -> numpy (H,W) u8, or into a device buffer given as int pointer"""
        if dst is None:
            out = np.empty((self.cfg.height, self.cfg.width), np.uint8)
            self._hd.check(self._hd.L.esvio_fe_export_image(self._hd.h, cam, _p(out), HOST))
            return out
        self._hd.check(self._hd.L.esvio_fe_export_image(self._hd.h, cam, C.c_void_p(int(dst)), DEVICE))
        return None

    def export_level(self, cam, level):
        """level `level` of the pyramid in the current slot of `cam`, with its border (esvio_fe_export_level) ->
        (image (h + 2 PAD, w + 2 PAD) u8, derivatives (h + 2 PAD, w + 2 PAD, 2) int16, the handle's top level)"""
        w, h, top = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._hd.check(self._hd.L.esvio_fe_export_level(self._hd.h, cam, level, None, None, C.byref(w), C.byref(h),
                                                        C.byref(top)))
        im = np.empty((h.value + 2 * PAD, w.value + 2 * PAD), np.uint8)
        dv = np.empty((h.value + 2 * PAD, w.value + 2 * PAD, 2), np.int16)
        self._hd.check(self._hd.L.esvio_fe_export_level(self._hd.h, cam, level, _p(im), _p(dv), C.byref(w), C.byref(h),
                                                        C.byref(top)))
        return im, dv, top.value

    def import_image(self, cam, src):
        """numpy (H,W) u8 or device pointer (int): right image for the next trackEvent"""
        if isinstance(src, np.ndarray):
            src = np.ascontiguousarray(src, np.uint8)
            self._hd.check(self._hd.L.esvio_fe_import_image(self._hd.h, cam, _p(src), HOST))
        else:
            self._hd.check(self._hd.L.esvio_fe_import_image(self._hd.h, cam, C.c_void_p(int(src)), DEVICE))

    # ---- stage-level entry points used by the parity tests
    def Event_FeaturesToTrack(self, last_event, maxCorners, event_mask=None):
        ptr, n, space, keep = _events_arg(last_event)
        xy = np.zeros((max(maxCorners, 1), 2), np.float32)
        idx = np.zeros(max(maxCorners, 1), np.int32)
        k = C.c_int32(0)
        mask = None if event_mask is None else np.ascontiguousarray(event_mask, np.uint8)
        self._hd.check(self._hd.L.esvio_fe_features_to_track(
            self._hd.h, ptr, n, space, int(maxCorners), _p(mask), _p(xy), _p(idx), C.byref(k)))
        return xy[:k.value].copy(), idx[:k.value].copy()

    def select_candidates(self, xy, payload, disc, euclid=False, table=False, mask=None, stamp_pts=None, max_corners=None,
                          out_base=0, variant=0, poison=None):
        """test tap (esvio_fe_select_candidates, include/esvio_fe_test.h): the greedy min-distance selection over the
        candidates xy (uint32 x | y << 16) with their int32 payloads.  disc: cv::circle's radius, or with euclid the
        min_distance of the open Euclidean disc; table: membership by the half-width table; mask: (H, W) u8, 255 =
        blocked; stamp_pts: float32 (k, 2) points whose discs are blocked; variant 0 / 1 / 2: the handle's kernel / the
        one-wave kernel / the bitmap in device memory.  poison = (float, int): what the output arrays hold before the
        call -> (out_xy float32 (max_cnt, 2), out_idx int32 (max_cnt), counts int32 (3), kernel name), the arrays WHOLE:
        the accepted points are out_xy[out_base : out_base + counts[0]], their payloads out_idx[: counts[0]]"""
        hd = self._hd
        M = self.cfg.max_cnt
        xy = np.ascontiguousarray(xy, np.uint32).reshape(-1)
        payload = np.ascontiguousarray(payload, np.int32).reshape(-1)
        if xy.size != payload.size:
            raise ValueError("one payload per candidate")
        st = None if stamp_pts is None else np.ascontiguousarray(stamp_pts, np.float32).reshape(-1, 2)
        mk = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        if mk is not None and mk.shape != (self.cfg.height, self.cfg.width):
            raise ValueError("mask must be (height, width) of the handle")
        pf, pi = (0.0, 0) if poison is None else poison
        out_xy = np.full((M, 2), pf, np.float32)
        out_idx = np.full(M, pi, np.int32)
        counts = np.zeros(3, np.int32)
        kid = C.c_int32(-1)
        flags = (SELECT_EUCLID if euclid else 0) | (SELECT_TABLE if table else 0)
        hd.check(hd.L.esvio_fe_select_candidates(
            hd.h, _p(xy) if xy.size else None, _p(payload) if xy.size else None, int(xy.size), float(disc), flags, _p(mk),
            _p(st) if st is not None and len(st) else None, 0 if st is None else len(st),
            M if max_corners is None else int(max_corners), int(out_base), int(variant), _p(out_xy), _p(out_idx), _p(counts),
            C.byref(kid)))
        return out_xy, out_idx, counts, hd.L.esvio_fe_kernel_name(kid.value).decode()

    def calcOpticalFlowPyrLK(self, prev_img, next_img, prev_pts, next_pts=None, maxLevel=3,
                             max_count=30, eps=0.01, flags=0):
        prev_img = np.ascontiguousarray(prev_img, np.uint8)
        next_img = np.ascontiguousarray(next_img, np.uint8)
        h, w = prev_img.shape
        prev_pts = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
        n = prev_pts.shape[0]
        nxt = (np.zeros((n, 2), np.float32) if next_pts is None
               else np.array(next_pts, np.float32).reshape(-1, 2).copy())
        status = np.zeros(n, np.uint8)
        self._hd.check(self._hd.L.esvio_fe_calc_optical_flow_pyr_lk(
            self._hd.h, _p(prev_img), _p(next_img), w, h, _p(prev_pts), _p(nxt), _p(status), n,
            maxLevel, max_count, eps, flags))
        return nxt, status

    def build_pyramid(self, img, max_level=3):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        nl, lw, lh = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._hd.check(self._hd.L.esvio_fe_build_pyramid(self._hd.h, _p(img), w, h, max_level, -1,
                                                         None, None, None, None, C.byref(nl)))
        levels = []
        for l in range(nl.value):
            self._hd.check(self._hd.L.esvio_fe_build_pyramid(
                self._hd.h, _p(img), w, h, max_level, l, None, None, C.byref(lw), C.byref(lh),
                C.byref(nl)))
            im = np.empty((lh.value, lw.value), np.uint8)
            dv = np.empty((lh.value, lw.value, 2), np.int16)
            self._hd.check(self._hd.L.esvio_fe_build_pyramid(
                self._hd.h, _p(img), w, h, max_level, l, _p(im), _p(dv), C.byref(lw), C.byref(lh),
                C.byref(nl)))
            levels.append((im, dv))
        return levels

    # ---- measurement
    def set_profiling(self, on=True):
        self._hd.check(self._hd.L.esvio_fe_set_profiling(self._hd.h, int(on)))

    def reset_kernel_stats(self):
        self._hd.check(self._hd.L.esvio_fe_reset_kernel_stats(self._hd.h))

    def kernel_stats(self, stages=False):
        """per kernel of the track paths (stages=True: and of the stages off them, esvio_fe_filter_events' k_baf_*)"""
        L = self._hd.L
        out = {}
        for k in range(L.esvio_fe_stage_kernel_count() if stages else L.esvio_fe_kernel_count()):
            ms, n, b = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
            self._hd.check(L.esvio_fe_get_kernel_stats(self._hd.h, k, C.byref(ms), C.byref(n),
                                                       C.byref(b)))
            out[L.esvio_fe_kernel_name(k).decode()] = dict(ms=ms.value, launches=n.value,
                                                           alg_bytes=b.value)
        return out

    @property
    def stream(self):
        return self._hd.L.esvio_fe_stream(self._hd.h)


def comm_unique_id():
    """ncclGetUniqueId through the library (rank 0); 128 bytes to hand to every rank's comm_init"""
    buf = (C.c_uint8 * 128)()
    rc = load_library().esvio_fe_comm_unique_id(buf)
    if rc:
        raise FrontendError("esvio_fe_comm_unique_id rc=%d (librccl.so not found?)" % rc)
    return bytes(buf)


class EventBuffer:
    """an event batch in memory from the library's own HIP runtime (esvio_fe_mem_alloc): pinned host memory
    (`.array`: a numpy view that can be passed wherever a host batch goes — it is DMA'd without the staging
    copy) or device memory (`.arg`: the (pointer, n) tuple the entry points take for ESVIO_FE_DEVICE)"""

    def __init__(self, events, space=HOST):
        ev = np.ascontiguousarray(events)
        assert ev.dtype.itemsize == 16
        self.space, self.n = space, len(ev)
        p = C.c_void_p()
        rc = load_library().esvio_fe_mem_alloc(space, ev.nbytes, C.byref(p))
        if rc:
            raise FrontendError("esvio_fe_mem_alloc rc=%d" % rc)
        self.ptr = p
        if space == HOST:
            raw = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(ev.nbytes, 16),))
            raw[:ev.nbytes] = ev.view(np.uint8).reshape(-1)
            self.array = raw[:ev.nbytes].view(ev.dtype)
        else:
            rc = load_library().esvio_fe_mem_upload(p, _p(ev), ev.nbytes)
            if rc:
                raise FrontendError("esvio_fe_mem_upload rc=%d" % rc)
            self.arg = (p.value, self.n)

    def free(self):
        if self.ptr:
            load_library().esvio_fe_mem_free(self.space, self.ptr)
            self.ptr = None
            self.array = None


class ConvertedEvents:
    """the records esvio_fe_convert_events made of an events.EventFields: in device memory of the library's runtime
    (`.arg`, the (pointer, n) tuple of ESVIO_FE_DEVICE) or downloaded (`.array`); EventBuffer's contract"""

    def __init__(self, hd, fields, space=DEVICE, src_space=HOST):
        from .events import EVENT_DTYPE
        self.space, self.n, self.ptr, self.array = space, fields.n, None, None
        L = hd.L
        if space == DEVICE:
            p = C.c_void_p()
            rc = L.esvio_fe_mem_alloc(DEVICE, 16 * max(self.n, 1), C.byref(p))
            if rc:
                raise FrontendError("esvio_fe_mem_alloc rc=%d" % rc)
            self.ptr, dst = p, p
        else:
            self.array = np.zeros(self.n, EVENT_DTYPE)
            dst = _p(self.array)
        bad = C.c_uint64(0)
        desc = fields_desc(fields)
        rc = L.esvio_fe_convert_events(hd.h, C.byref(desc), self.n, src_space, dst, space, C.byref(bad))
        if rc:
            self.free()
            e = FrontendError("rc=%d: %s" % (rc, L.esvio_fe_last_error(hd.h).decode()))
            e.n_bad = int(bad.value)
            raise e
        if space == DEVICE:
            self.arg = (self.ptr.value, self.n)

    def free(self):
        if self.ptr:
            load_library().esvio_fe_mem_free(DEVICE, self.ptr)
            self.ptr = None
        self.array = None


class FilteredEvents:
    """the records esvio_fe_filter_events kept, in device memory of the library's runtime: `.arg` is the (pointer, n)
    tuple of ESVIO_FE_DEVICE, `.last` the last kept record (None if there is none)"""

    def __init__(self, ptr, n, last):
        self.space, self.ptr, self.n, self.last = DEVICE, ptr, n, last
        self.arg = (ptr.value, n)

    def free(self):
        if self.ptr:
            load_library().esvio_fe_mem_free(DEVICE, self.ptr)
            self.ptr = None


class DeviceImages:
    """n dense width x height gray images side by side in device memory of the library's runtime (what
    esvio_fe_decode_bag_images, esvio_fe_decode_aedat_frames and the two conversions write): `.image(k)` is the k-th one's address, which
    trackImage(..., device=True) takes; `.download()` brings them to the host"""

    def __init__(self, ptr, n, width, height):
        self.space, self.ptr, self.n, self.width, self.height = DEVICE, ptr, n, width, height

    def image(self, k):
        assert 0 <= k < self.n
        return self.ptr.value + int(k) * self.width * self.height

    def download(self):
        out = np.zeros((self.n, self.height, self.width), np.uint8)
        if out.nbytes:
            hip = C.CDLL("libamdhip64.so")
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            rc = hip.hipMemcpy(_p(out), self.ptr, out.nbytes, 2)
            if rc:
                raise FrontendError("hipMemcpy rc=%d" % rc)
        return out

    def free(self):
        if self.ptr:
            load_library().esvio_fe_mem_free(DEVICE, self.ptr)
            self.ptr = None


class RegisteredEvents:
    """a caller-owned numpy event array page-locked where it lies (esvio_fe_register_host_buffer): batches handed
    over from it cross PCIe without the staging copy; `.array` is the array itself"""

    def __init__(self, events):
        self.array = np.ascontiguousarray(events)
        assert self.array.dtype.itemsize == 16 and len(self.array)
        rc = load_library().esvio_fe_register_host_buffer(_p(self.array), self.array.nbytes)
        if rc:
            raise FrontendError("esvio_fe_register_host_buffer rc=%d" % rc)
        self.registered = True

    def free(self):
        if self.registered:
            load_library().esvio_fe_unregister_host_buffer(_p(self.array))
            self.registered = False


def host_nullspace(systems, lanes):
    """run7Point's null-space basis of n 7x9 systems -> (f[n, 2, 9], systems redone one at a time);
    lanes False: the one-at-a-time routine, True: the vector-lane form the RANSAC loop uses"""
    a = np.ascontiguousarray(systems, np.float64).reshape(-1, 7, 9)
    f = np.empty((a.shape[0], 2, 9), np.float64)
    redone = C.c_int32(0)
    rc = load_library().esvio_fe_host_nullspace(_p(a), a.shape[0], int(bool(lanes)), _p(f), C.byref(redone))
    if rc != 0:
        raise FrontendError("host_nullspace rc=%d" % rc)
    return f, redone.value


def host_hypot(x, y):
    """the hypot of the 7-point solver's Jacobi rotations: cv::hypot of OpenCV's lapack.cpp, a*sqrt(1+(b/a)^2)"""
    x = np.ascontiguousarray(x, np.float64)
    y = np.ascontiguousarray(y, np.float64)
    out = np.empty_like(x)
    rc = load_library().esvio_fe_host_hypot(_p(x), _p(y), x.size, _p(out))
    if rc != 0:
        raise FrontendError("host_hypot rc=%d" % rc)
    return out


def ransac_stats(reset=False):
    """process-wide counters of the host findFundamentalMat: RANSAC branch dict(calls, iterations,
    points, us) + LMedS branch (lmeds_calls, lmeds_us)"""
    out = (C.c_uint64 * 6)()
    L = load_library()
    rc = L.esvio_fe_ransac_stats(out, 1 if reset else 0)
    if rc != 0:
        raise FrontendError("ransac_stats rc=%d" % rc)
    return {"calls": int(out[0]), "iterations": int(out[1]), "points": int(out[2]), "us": out[3] / 1e3,
            "lmeds_calls": int(out[4]), "lmeds_us": out[5] / 1e3}


def ransac_tail(reset=False):
    """the tail of the host findFundamentalMat (process-wide): slowest RANSAC / LMedS call [us], iterations the
    calling thread redid for a helper that did not deliver, jobs run without the helpers, jobs that took the
    other job buffer because a helper was stuck in theirs, involuntary context switches of the helper threads"""
    out = (C.c_uint64 * 6)()
    rc = load_library().esvio_fe_ransac_tail(out, 1 if reset else 0)
    if rc != 0:
        raise FrontendError("ransac_tail rc=%d" % rc)
    return {"max_us": out[0] / 1e3, "lmeds_max_us": out[1] / 1e3, "redone_iterations": int(out[2]),
            "solo_jobs": int(out[3]), "skipped_buffers": int(out[4]), "helper_invol_switches": int(out[5])}


def find_fundamental_mat(p1, p2, thr=1.0, conf=0.99, threads=1, hold_mask=None):
    """cv::findFundamentalMat(p1, p2, FM_RANSAC, thr, conf, status) (host-side stage).  hold_mask (test tap,
    threads >= 2): job buffers of the helper pool marked as still holding a descheduled helper"""
    L = load_library()
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
    n = p1.shape[0]
    status = np.zeros(n, np.uint8)
    k = C.c_int32(0)
    if hold_mask is not None:
        rc = L.esvio_fe_find_fundamental_mat_held(_p(p1), _p(p2), n, thr, conf, threads, int(hold_mask), _p(status),
                                                  C.byref(k))
    elif threads > 1:
        rc = L.esvio_fe_find_fundamental_mat_mt(_p(p1), _p(p2), n, thr, conf, threads, _p(status),
                                                C.byref(k))
    else:
        rc = L.esvio_fe_find_fundamental_mat(_p(p1), _p(p2), n, thr, conf, _p(status), C.byref(k))
    if rc:
        raise FrontendError("find_fundamental_mat rc=%d" % rc)
    return k.value, status


def find_fundamental_mat_idle(p1, p2, thr=1.0, conf=0.99, threads=4, repeats=4, idle_units=64):
    """test tap: findFundamentalMat on a helper pool whose helpers are handed other work between jobs (what the
    host-batch staging does) -> (inliers, status, {idle_calls, idle_done, idle_left})"""
    L = load_library()
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
    n = p1.shape[0]
    status = np.zeros(n, np.uint8)
    k = C.c_int32(0)
    out = (C.c_uint64 * 3)()
    rc = L.esvio_fe_find_fundamental_mat_idle(_p(p1), _p(p2), n, thr, conf, threads, repeats, idle_units, _p(status),
                                              C.byref(k), out)
    if rc:
        raise FrontendError("find_fundamental_mat_idle rc=%d" % rc)
    return k.value, status, dict(idle_calls=int(out[0]), idle_done=int(out[1]), idle_left=int(out[2]))


def raw_header(data):
    """a .raw file's ASCII header (esvio_fe_raw_header; host only, no handle): `data` the file's first bytes.  Returns
    the RawHeaderInfo: .payload_offset, .format (RAW_EVT2 / RAW_EVT21 / RAW_EVT3, 0: unknown), .width / .height
    (0: unknown), .complete (0: the header's end is not inside `data` — read more and call again)"""
    buf = bytes(data)
    info = RawHeaderInfo()
    rc = load_library().esvio_fe_raw_header(buf if buf else None, len(buf), C.byref(info))
    if rc:
        raise FrontendError("esvio_fe_raw_header rc=%d" % rc)
    return info


def text_imu(data, t_offset_ns=0, cap=None):
    """an imu.txt of the davis extractor, "t ax ay az gx gy gz" (esvio_fe_text_imu; host only, no handle): the whole
    file's bytes.  Returns a numpy IMU_DTYPE array; cap None: one sample per 14 bytes.  A line that does not read raises
    FrontendError with `.n` = the samples in front of it (too small a cap: the number needed)."""
    buf = bytes(data)
    cap = len(buf) // 14 + 1 if cap is None else int(cap)
    out, n = np.zeros(max(cap, 1), IMU_DTYPE), C.c_size_t(0)
    rc = load_library().esvio_fe_text_imu(buf if buf else None, len(buf), int(t_offset_ns), _p(out), cap, C.byref(n))
    if rc:
        e = FrontendError("esvio_fe_text_imu rc=%d" % rc)
        e.n = int(n.value)
        raise e
    return out[:n.value]


def text_images(data, t_offset_ns=0, cap=None):
    """an images.txt of the davis extractor, "t path" (esvio_fe_text_images; host only, no handle).  Returns (stamps_ns, paths):
    an int64 numpy array and a list of bytes.  Failures as text_imu's."""
    buf = bytes(data)
    cap = len(buf) // 4 + 1 if cap is None else int(cap)
    st, off, ln, n = np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint32), C.c_size_t(0)
    rc = load_library().esvio_fe_text_images(buf if buf else None, len(buf), int(t_offset_ns), _p(st), _p(off), _p(ln), cap, C.byref(n))
    if rc:
        e = FrontendError("esvio_fe_text_images rc=%d" % rc)
        e.n = int(n.value)
        raise e
    k = int(n.value)
    return st[:k], [buf[int(o):int(o) + int(m)] for o, m in zip(off[:k], ln[:k])]


def text_limits():
    """esvio_fe_text_limits (include/esvio_fe_test.h): .tile_bytes, .max_body, .max_tail"""
    out = TextLimits()
    load_library().esvio_fe_text_limits(C.byref(out))
    return out


def scan_lanes():
    """esvio_fe_scan_lanes (include/esvio_fe_test.h): the lanes of each ingest chain's top scan, .raw, .aedat, .text, .slice,
    .filter, .pick, and the two tile sizes no other tap returns, .filter_block_events, .pick_tile_values"""
    out = ScanLanes()
    assert load_library().esvio_fe_scan_lanes(C.byref(out)) == 0
    return out


def lift_projective(cam, u, v):
    L = load_library()
    c = Camera(**{k: float(cam[k]) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")})
    out = np.empty(3, np.float64)
    rc = L.esvio_fe_lift_projective(C.byref(c), float(u), float(v), _p(out))
    if rc:
        raise FrontendError("lift_projective rc=%d" % rc)
    return out


def aedat_header(data):
    """an AEDAT recording's text header (esvio_fe_aedat_header; host only, no handle): `data` the file's first bytes.
    Returns the AedatHeaderInfo: .payload_offset, .version (31: AEDAT 3.1; 0: not stated), .complete."""
    buf = bytes(data)
    info = AedatHeaderInfo()
    rc = load_library().esvio_fe_aedat_header(buf if buf else None, len(buf), C.byref(info))
    if rc:
        raise FrontendError("esvio_fe_aedat_header rc=%d" % rc)
    return info


def aedat_walk_tap(state, data, runs_cap=None, events_cap=None):
    """the AEDAT host walk alone (esvio_fe_aedat_walk_tap; include/esvio_fe_test.h): `state` a bytes object (None: the
    fresh state).  Returns (state, runs, payload, counts): runs an (n, 2) int64 array of (first record, overflow),
    payload the packed 8-byte records as bytes, counts = (records, runs, polarity packets, other packets).  A malformed
    header raises FrontendError."""
    L = load_library()
    nst = L.esvio_fe_aedat_walk_state_bytes()
    st = np.zeros(nst, np.uint8) if state is None else np.frombuffer(bytes(state), np.uint8).copy()
    buf = np.frombuffer(bytes(data), np.uint8)
    events_cap = buf.nbytes // 8 + 1 if events_cap is None else events_cap
    runs_cap = events_cap if runs_cap is None else runs_cap
    runs, pay, counts = np.zeros((max(runs_cap, 1), 2), np.uint32), np.zeros(max(events_cap, 1) * 8, np.uint8), np.zeros(4, np.uint64)
    rc = L.esvio_fe_aedat_walk_tap(_p(st), nst, _p(buf) if buf.nbytes else None, buf.nbytes, _p(runs), runs_cap, _p(pay), events_cap, _p(counts))
    if rc:
        raise FrontendError("esvio_fe_aedat_walk_tap rc=%d" % rc)
    n, nr = int(counts[0]), int(counts[1])
    r = np.stack([runs[:nr, 0].astype(np.int64), runs[:nr, 1].view(np.int32).astype(np.int64)], axis=1) if nr else np.zeros((0, 2), np.int64)
    return st.tobytes(), r, pay[:8 * n].tobytes(), tuple(int(v) for v in counts)


def _bag_topics(left, right, imu):
    enc = lambda t: None if t is None else (t if isinstance(t, bytes) else str(t).encode())
    return BagTopics(enc(left), enc(right), enc(imu))


def bag_header(data):
    """a rosbag's magic and bag header record (esvio_fe_bag_header; host only, no handle): `data` the file's first bytes.
    Returns the BagHeaderInfo: .payload_offset (13: where the walkers start), .index_pos, .conn_count, .chunk_count,
    .version (20), .complete.  Bytes that are no bag raise FrontendError."""
    buf = bytes(data)
    info = BagHeaderInfo()
    rc = load_library().esvio_fe_bag_header(buf if buf else None, len(buf), C.byref(info))
    if rc:
        raise FrontendError("esvio_fe_bag_header rc=%d" % rc)
    return info


def bag_walk_tap(state, data, topics=(None, None, None), side=False, events_cap=None, msgs_cap=None, imu_cap=None):
    """the rosbag host walk alone (esvio_fe_bag_walk_tap; include/esvio_fe_test.h): `state` a bytes object (None: the
    fresh state), topics = (left, right, imu).  Returns (state, (left, right), messages, imu, counts): each camera's
    gathered 13-byte wire events as bytes, numpy BAG_MESSAGE_DTYPE and IMU_DTYPE arrays (what there was room for), the
    twelve counts.  A malformed
    stream raises FrontendError whose text is the broken rule."""
    L = load_library()
    nst = L.esvio_fe_bag_walk_state_bytes()
    st = np.zeros(nst, np.uint8) if state is None else np.frombuffer(bytes(state), np.uint8).copy()
    buf = np.frombuffer(bytes(data), np.uint8)
    events_cap = buf.nbytes // 13 + 1 if events_cap is None else events_cap
    msgs_cap = buf.nbytes // 28 + 1 if msgs_cap is None else msgs_cap
    imu_cap = buf.nbytes // 296 + 1 if imu_cap is None else imu_cap
    pay = [np.zeros(max(events_cap, 1) * 13, np.uint8) for _ in range(2)]
    msgs, imu, counts = np.zeros(max(msgs_cap, 1), BAG_MESSAGE_DTYPE), np.zeros(max(imu_cap, 1), IMU_DTYPE), np.zeros(12, np.uint64)
    why = C.create_string_buffer(512)
    ptrs = (C.c_void_p * 2)(pay[0].ctypes.data, pay[1].ctypes.data)
    rc = L.esvio_fe_bag_walk_tap(_p(st), nst, C.byref(_bag_topics(*topics)), int(bool(side)), _p(buf) if buf.nbytes else None, buf.nbytes,
                                 C.byref(ptrs), C.byref((C.c_size_t * 2)(events_cap, events_cap)), _p(msgs), msgs_cap, _p(imu), imu_cap,
                                 _p(counts), why, len(why))
    if rc:
        raise FrontendError("esvio_fe_bag_walk_tap rc=%d: %s" % (rc, why.value.decode()))
    c = tuple(int(v) for v in counts)
    return (st.tobytes(), tuple(pay[k][:13 * min(c[k], events_cap)].tobytes() for k in range(2)), msgs[:min(c[4], msgs_cap)].copy(),
            imu[:min(c[5], imu_cap)].copy(), c)


def aedat_frame_walk_tap(state, data, size=(0, 0), t_offset_ns=0, flags=0, pix_cap=None, frames_cap=None):
    """the AEDAT host walk in its frame mode alone (esvio_fe_aedat_frame_walk_tap; include/esvio_fe_test.h): `state` a
    (walker bytes, waiting pixel bytes) pair (None: the fresh state), size = (width, height) the only size taken ((0, 0):
    any).  Returns (state, pix, table, counts): the gathered pixel bytes, each frame from a 16-byte boundary, as bytes, a
    numpy AEDAT_FRAME_DTYPE array (what there was room for), the eight counts.  A malformed stream, a refused frame or a
    BAD stamp raises FrontendError whose text is the broken rule."""
    L = load_library()
    nst = L.esvio_fe_aedat_walk_state_bytes()
    st = np.zeros(nst, np.uint8) if state is None else np.frombuffer(bytes(state[0]), np.uint8).copy()
    waiting = b"" if state is None else bytes(state[1])
    buf = np.frombuffer(bytes(data), np.uint8)
    carry = np.zeros(len(waiting) + buf.nbytes + 1, np.uint8)
    carry[:len(waiting)] = np.frombuffer(waiting, np.uint8)
    pix_cap = len(waiting) + buf.nbytes + 16 * (buf.nbytes // 38 + 2) if pix_cap is None else int(pix_cap)
    frames_cap = buf.nbytes // 38 + 1 if frames_cap is None else int(frames_cap)
    pix, table, counts = np.zeros(max(pix_cap, 1), np.uint8), np.zeros(max(frames_cap, 1), AEDAT_FRAME_DTYPE), np.zeros(8, np.uint64)
    why = C.create_string_buffer(256)
    rc = L.esvio_fe_aedat_frame_walk_tap(_p(st), nst, int(size[0]), int(size[1]), _p(buf) if buf.nbytes else None, buf.nbytes, int(t_offset_ns),
                                         int(flags), _p(carry), len(carry), _p(pix), pix_cap, _p(table), frames_cap, _p(counts), why, len(why))
    if rc:
        raise FrontendError("esvio_fe_aedat_frame_walk_tap rc=%d: %s" % (rc, why.value.decode()))
    c = tuple(int(v) for v in counts)
    return (st.tobytes(), carry[:c[6]].tobytes()), pix[:c[1]].tobytes() if c[1] <= pix_cap else b"", table[:min(c[0], frames_cap)], c


def bag_image_walk_tap(state, data, topics=(None, None), size=(0, 0), pix_cap=None, imgs_cap=None):
    """the rosbag host walk in its image mode alone (esvio_fe_bag_image_walk_tap; include/esvio_fe_test.h): `state` a
    (walker bytes, waiting payload bytes) pair (None: the fresh state), topics = (left, right), size = (width, height)
    the only size taken ((0, 0): any).  Returns (state, pix, table, counts): the gathered payloads, each from a 16-byte
    boundary, as bytes, a numpy BAG_IMAGE_DTYPE array (what there was room for), the twelve counts.  A malformed stream
    or a refused message raises FrontendError whose text is the broken rule."""
    L = load_library()
    nst = L.esvio_fe_bag_walk_state_bytes()
    st = np.zeros(nst, np.uint8) if state is None else np.frombuffer(bytes(state[0]), np.uint8).copy()
    waiting = b"" if state is None else bytes(state[1])
    buf = np.frombuffer(bytes(data), np.uint8)
    carry = np.zeros(len(waiting) + buf.nbytes + 1, np.uint8)
    carry[:len(waiting)] = np.frombuffer(waiting, np.uint8)
    pix_cap = len(waiting) + buf.nbytes + 16 * (buf.nbytes // 38 + 2) if pix_cap is None else int(pix_cap)
    imgs_cap = buf.nbytes // 38 + 1 if imgs_cap is None else int(imgs_cap)
    pix, imgs, counts = np.zeros(max(pix_cap, 1), np.uint8), np.zeros(max(imgs_cap, 1), BAG_IMAGE_DTYPE), np.zeros(12, np.uint64)
    why = C.create_string_buffer(512)
    enc = lambda t: None if t is None else (t if isinstance(t, bytes) else str(t).encode())
    rc = L.esvio_fe_bag_image_walk_tap(_p(st), nst, enc(topics[0]), enc(topics[1]), int(size[0]), int(size[1]), _p(buf) if buf.nbytes else None,
                                       buf.nbytes, _p(carry), len(carry), _p(pix), pix_cap, _p(imgs), imgs_cap, _p(counts), why, len(why))
    if rc:
        raise FrontendError("esvio_fe_bag_image_walk_tap rc=%d: %s" % (rc, why.value.decode()))
    c = tuple(int(v) for v in counts)
    return ((st.tobytes(), carry[:c[8]].tobytes()), pix[:c[3]].tobytes() if c[3] <= pix_cap else b"", imgs[:min(c[0], imgs_cap)], c)  # (a view: a copy would drop the row's padding word)
